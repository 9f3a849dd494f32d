"""All 256 byte values in and beside the ASCII input of every search kernel path (-m gpu): the _async entry points that came after
tests/test_gpu_alphabet.py -- along a reference the Hamming best match and histogram, the pattern hit list and count, the edit-distance best match,
count and hit list; per read the Hamming best match, runner-up and ragged batch, the anchored matchers (Hamming, edit distance, patterns; fixed and
ragged batches) and the whole-read edit-distance matchers.

One test per path, through tests/test_gpu_alphabet.py's run_path, so every path gets ACCEPT (upper, lower and mixed case give the oracle's result),
REJECT (alphabet.reject_plan: each of the 248 invalid values once at each byte lane, 992 cases rotating over the path's regions; the error is the
first invalid OWNED byte in buffer order, a later one of the other class never wins, the next sync is clean, one clean call follows the sweep) and
IGNORE (the bytes the entry point does not own -- around the batch, outside the spans, inside reads without a span or shorter than k -- take each of
the 256 values: the call succeeds with the oracle's result and the guard bytes around all outputs stay untouched).  Where a layout has bytes between
owned ranges a gap variant on a larger batch follows: every value directly before and directly after an owned range at every byte lane, in one call.

The paths -- shapes, owned and foreign positions (from the header's validation paragraphs), regions (from the kernels' constants) and expected values
(from the family oracles) -- are tests/alphabet_search.py's; tests/test_alphabet_classes.py checks their plans without a GPU.  Several paths carry
17 queries (two query blocks) or 5 (an interleave group of four and one of one): only the first may report an invalid byte, which REJECT's "reported
once" and the exact (byte, index) both hold it to."""
import numpy as np
import pytest

import alphabet_search as als
from test_gpu_alphabet import Out, Path, Src, run_path

pytestmark = pytest.mark.gpu


def device_path(ctx, oracle, spec):
    """the Spec's inputs and outputs on the device -> (Path, {input name: (tensor, the array it was made from)})"""
    import torch
    dev = {name: (torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda(), a) for name, a in spec.inputs.items()}
    ptrs = {name: t.data_ptr() for name, (t, _) in dev.items()}
    assert all(p % 16 == 0 for p in ptrs.values())
    outs = [Out(nbytes, off) for nbytes, off in spec.outs]
    optrs = [o.ptr for o in outs]
    P = Path(spec.name, spec.good, spec.off, spec.regions, outs, lambda ptr: spec.call(ctx, ptr, ptrs, optrs), lambda s: spec.want(oracle, s),
             owned=spec.owned, foreign=spec.foreign, keep=(dev, spec))
    P.unpolluted = spec.unpolluted
    assert isinstance(P.src, Src) and P.src.clean.numel() == spec.good.size + spec.off + 2 * 256  # the 256-byte pads on both sides
    return P, dev


@pytest.mark.parametrize("path", list(als.PATHS))
def test_search_path(ctx, oracle, path):
    make, make_gap = als.PATHS[path]
    P, dev = device_path(ctx, oracle, make())
    G, gdev = device_path(ctx, oracle, make_gap()) if make_gap else (None, {})
    run_path(ctx, oracle, P, gap=G)
    for name, (t, a) in list(dev.items()) + list(gdev.items()):  # queries, patterns, thresholds and tables are inputs: left as they were
        assert np.array_equal(t.cpu().numpy(), np.ascontiguousarray(a).view(np.uint8).reshape(-1)), name
