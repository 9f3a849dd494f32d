"""CPU-only: the oracle (scalar + AVX2 restatements) under ASan + UBSan with exact-size heap
buffers.  GPU AddressSanitizer is not available on this pool; the device side is covered by
guard-word checks in tests/test_gpu_parity.py."""
import os
import platform
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "oracle_sanitize")
    cmd = ["gcc", "-O1", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-march=x86-64-v3",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "c", "oracle_sanitize.c"),
           os.path.join(ROOT, "oracle", "bitnuc_oracle.c"), os.path.join(ROOT, "oracle", "bitnuc_avx2.c"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sanitizer harness ok" in out.stdout


def _build_and_run_host_harness(tmp_path, tag, san_flags, env_extra, no_aslr=False):
    exe = str(tmp_path / f"host_sanitize_{tag}")
    obj = str(tmp_path / f"oracle_{tag}.o")
    subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", *san_flags, "-c",
                    os.path.join(ROOT, "oracle", "bitnuc_oracle.c"), "-o", obj], check=True, capture_output=True)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", *san_flags, os.path.join(ROOT, "tests", "c", "host_sanitize.cpp"), obj, "-o", exe, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, **env_extra)
    out = None
    setarch = shutil.which("setarch")
    if no_aslr and setarch:  # this process only: address randomisation off (the machine's setting is untouched)
        out = subprocess.run([setarch, platform.machine(), "-R", exe], capture_output=True, text=True, timeout=900, env=env)
        if out.stderr.startswith("setarch:"):  # the personality call itself was refused: run as is
            out = None
    if out is None:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-6000:]
    assert "host sanitizer harness ok" in out.stdout


def test_product_host_code_under_asan_ubsan(tmp_path):
    """The product's own CPU code -- csrc/host_word.h (single words, below-cutoff bulk calls) and csrc/host_pool.h (the mover
    thread of the pipelined host-pointer path) -- under AddressSanitizer + UBSan: exact-size heap buffers, every length, the
    mover in pipe_run's call pattern.  Both headers compile without HIP."""
    _build_and_run_host_harness(tmp_path, "asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                                {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0"})


def test_product_host_pool_under_tsan(tmp_path):
    """The same harness under ThreadSanitizer: the mover thread's mutex / condition-variable protocol (tickets, waits for a
    ticket, drains, destruction with tasks queued) has no data race.  The harness runs with address randomisation off: this
    compiler's TSan runtime knows a fixed memory layout, and on kernels with 32 bits of mmap randomisation the executable can
    land outside it ("FATAL: ThreadSanitizer: unexpected memory mapping") before a line of the harness runs."""
    _build_and_run_host_harness(tmp_path, "tsan", ["-fsanitize=thread"], {"TSAN_OPTIONS": "halt_on_error=1:second_deadlock_stack=1"}, no_aslr=True)
