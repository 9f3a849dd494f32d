"""The byte classes of the ASCII entry points and the plan that walks them through a kernel path (no GPU; tests/test_alphabet_classes.py checks it).

Every entry point that reads ASCII bases accepts exactly the eight bytes of b"ACGTacgt" (src/utils/packing/naive.rs:10-16).  The register-level
validators all index an 8-entry table with the byte's low three bits and cancel the high bits under a mask, so the 248 other bytes fall into two
classes: those whose low three bits no base has (the table alone refuses them) and those that share their low three bits with a base (only the
high-bit residue under its mask refuses them; the IUPAC codes Y S W K D are among these).  The classes below come from the alphabet itself, not
from any kernel's constants."""
from math import gcd

import numpy as np

VALID = tuple(sorted(b"ACGTacgt"))
VALID_SELECTORS = frozenset(b & 7 for b in VALID)  # the low three bits some base has
INVALID_VALID_SELECTOR = tuple(b for b in range(256) if b not in VALID and (b & 7) in VALID_SELECTORS)
INVALID_OTHER = tuple(b for b in range(256) if b not in VALID and (b & 7) not in VALID_SELECTORS)
INVALID = tuple(sorted(INVALID_VALID_SELECTOR + INVALID_OTHER))
CLASS_OF = {**{b: "valid" for b in VALID}, **{b: "valid-selector" for b in INVALID_VALID_SELECTOR}, **{b: "other" for b in INVALID_OTHER}}

LUT = np.frombuffer(b"ACGT", dtype=np.uint8)

# The kernels' tiling constants the region layouts of tests/test_gpu_alphabet.py are derived from: name -> (value, source file under bitnuc_amd/csrc).
# tests/test_alphabet_classes.py::test_kernel_constants_match_the_sources reads them back from the sources' text.
KERNEL_CONSTANTS = {
    "kBlock": (256, "device_prims.h"),            # k-mers per workgroup trip of kmer_batch_kernel
    "kScanWaveWindows": (992, "kmer_device.h"),   # bases a round of kmer_scan_kernel / kmer_slide_kernel / kmer_slide_any_kernel advances by
    "kStagedMaxStride": (64, "kmer_device.h"),    # largest stride kmer_batch_kernel<true> stages through LDS
    "kSlide2Rounds": (4, "runtime.h"),            # 1 KiB rounds per trip
    "kScanSegRounds": (4, "runtime.h"),
    "kCountRounds": (4, "runtime.h"),
    "kHitsRounds": (4, "scan_hits_device.h"),
    "kMultiRounds": (4, "scan_multi_device.h"),
    "kMultiQB": (16, "scan_multi_device.h"),      # queries per query block (grid.y)
    "kBatchTile": (64, "batch_device.h"),         # words per wave tile of the read batches
    # the search kernels of tests/test_gpu_alphabet_search.py (shapes and regions: tests/alphabet_search.py)
    "kEdistRefChunk": (1024, "scan_edist_ref_device.h"),  # reported columns per lane of the edit-distance search along a reference
    "kEdistRefLead": (64, "scan_edist_ref_device.h"),     # columns a lane runs in front of its chunk: the lane of the chunk before reads them too
    "kEdistRefTrip": (64, "scan_edist_ref_device.h"),     # columns per trip: four 16-byte loads, byte by byte in the buffer's last trip
    "kEdistBlock": (256, "scan_edist_device.h"),          # reads per workgroup of the per-read edit-distance kernels, one per lane
    "kAnchorBlock": (256, "scan_anchored_device.h"),      # four waves of ...
    "kAnchorGroups": (2, "scan_anchored_device.h"),       # ... two groups of 32 reads each: 64 reads per wave
    "kReadsMinPeriod": (32, "scan_reads_device.h"),       # reads shorter than this run no rounds: one window per thread
    "kEdistInterleave": (4, "edist_step_device.h"),       # queries a lane walks side by side: Q = 5 is a group of four and a group of one
}
GROUP = 16     # bytes per lane load: the unit every register-level validator flags and rescan_bytes re-reads
ROUND = 1024   # bases per line-aligned round (scan_rounds in scan_mfma_host.h: round r reads bytes [1024 r, 1024 r + 1056))
HALO = 32      # the bytes after a round that its last windows read
ROUND992 = KERNEL_CONSTANTS["kScanWaveWindows"][0]
TRIP = 4       # rounds per trip of every line-aligned kernel (the five k*Rounds above)
TILE_WORDS = KERNEL_CONSTANTS["kBatchTile"][0]
ENCODE_TILE = 128 * 2 * GROUP  # bytes per workgroup tile of the shipped encode variant (codec.hip: X(39, 2, 128, ...): UNROLL x BLOCK groups)


def scan_rounds(n, skip=0):
    """scan_mfma_host.h: whole rounds of 1024 windows in n bases whose first `skip` are left to the head"""
    nr = max(n - skip, 0)
    return (nr - HALO) >> 10 if nr >= ROUND + HALO else 0


def rounds992(span):
    """kmer.hip: whole rounds of the 992-base kernels in `span` bytes (round r reads bytes [992 r, 992 r + 1024))"""
    return (span - ROUND) // ROUND992 + 1 if span >= ROUND else 0


def describe(byte):
    c = chr(byte) if 32 < byte < 127 else "."
    return f"0x{byte:02X} '{c}' ({CLASS_OF[byte]})"


def other_class(byte, salt):
    """An invalid byte of the class `byte` is not in (the second byte a reject case plants later in the input)."""
    pool = INVALID_OTHER if CLASS_OF[byte] == "valid-selector" else INVALID_VALID_SELECTOR
    return pool[salt % len(pool)]


def bases(rng, n, case="mixed"):
    """n random bases; case: "upper", "lower" or "mixed" (every base lower case with probability 1/2)."""
    s = LUT[rng.integers(0, 4, n)]
    if case == "lower":
        return (s | 0x20).astype(np.uint8)
    if case == "mixed":
        return np.where(rng.random(n) < 0.5, s | 0x20, s).astype(np.uint8)
    return s.astype(np.uint8)


def recase(s, case, seed=0):
    """The same bases in upper case, lower case or a seeded mix."""
    up = (s & 0xDF).astype(np.uint8)
    if case == "upper":
        return up
    if case == "lower":
        return (up | 0x20).astype(np.uint8)
    return np.where(np.random.default_rng(seed).random(s.size) < 0.5, up | 0x20, up).astype(np.uint8)


def reject_plan(regions):
    """regions: [(name, positions)] -- at most four code regions of one kernel path, each the positions (ints, any order) at which a byte of the
    input is examined by that region.  Yields (byte, position, region name): every invalid byte value once at each of the four byte lanes of a
    dword (position % 4), 248 x 4 = 992 cases.  Value i at lane l goes to region (i + l) mod R, so with R <= 4 every region sees every value; inside
    a region the positions of one lane are walked from the region's first to its last candidate with an odd step, so position % 16 takes all four
    residues that lane has."""
    if not 1 <= len(regions) <= 4:
        raise ValueError("one to four regions: every value has four cases, one per lane")
    cand = []
    for name, pos in regions:
        p = np.unique(np.asarray(list(pos), dtype=np.int64))
        lanes = [p[p % 4 == lane] for lane in range(4)]
        if any(x.size == 0 for x in lanes):
            raise ValueError(f"region {name!r} has no position at some byte lane")
        cand.append((name, lanes))
    seen = {}
    for lane in range(4):
        for i, byte in enumerate(INVALID):
            r = (i + lane) % len(cand)
            name, lanes = cand[r]
            c = lanes[lane]
            t = seen.get((r, lane), 0)
            seen[(r, lane)] = t + 1
            if t == 1:
                idx = c.size - 1  # the region's last candidate of this lane right after its first
            else:
                step = max(1, c.size // 61) | 1
                while gcd(step, c.size) != 1:
                    step += 2
                idx = (t * step) % c.size
            yield byte, int(c[idx]), name
