"""Helpers shared by tests/test_linesctx_host.py and tests/test_linesctx_gpu.py: the two context calls over poisoned arrays with guard
entries behind `capacity`, results in the shape of tests/linesctx_ref.py's model.  Test infrastructure only."""

import numpy as np

from pfac_amd import api

GUARD = 64
POISON = -7


def flags_of(invert):
    return api.PFACX_LINES_INVERT if invert else 0


def host_context(h, data, before, after, invert=False, with_index=True, with_tag=True):
    """matchLinesContextFromHost, capacity == size -> (start, len, index, tag, counts); the entries at and beyond capacity and the input
    must stay untouched, and so must an array that was passed as NULL"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    n = int(buf.size)
    arrays = [np.full(n + GUARD, POISON, dtype=np.int32) for _ in range(4)]
    start, length, index, tag = arrays
    st, nl, ns, nm, ng = h.matchLinesContextFromHost(buf.ctypes.data if n else start.ctypes.data, n, flags_of(invert), before, after,
                                                     start.ctypes.data, length.ctypes.data, index.ctypes.data if with_index else None,
                                                     tag.ctypes.data if with_tag else None, n)
    assert st == 0 and ng <= nm <= ns <= nl <= n
    assert all(np.all(a[n:] == POISON) for a in arrays), "wrote at or beyond capacity"
    assert buf.tobytes() == bytes(data), "the caller's input was modified"
    assert with_index or np.all(index == POISON)
    assert with_tag or np.all(tag == POISON)
    return start[:ns].copy(), length[:ns].copy(), index[:ns].copy(), tag[:ns].copy(), (nl, ns, nm, ng)


def device_context(h, data, before, after, invert=False, in_offset=0, with_index=True, with_tag=True, keep=False):
    """matchLinesContextFromDevice, capacity == size -> (start, len, index, tag, counts); keep: also the device tensors (input, offset,
    start, len) for a gather"""
    import torch
    data = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)
    n = int(data.size)
    d_in = torch.zeros(n + in_offset + 64, dtype=torch.uint8, device="cuda:0")
    d_in[in_offset:in_offset + n] = torch.from_numpy(data.copy()).to("cuda:0")
    tensors = [torch.full((n + GUARD,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(4)]
    d_start, d_len, d_index, d_tag = tensors
    st, nl, ns, nm, ng = h.matchLinesContextFromDevice(d_in.data_ptr() + in_offset, n, flags_of(invert), before, after, d_start.data_ptr(),
                                                       d_len.data_ptr(), d_index.data_ptr() if with_index else None,
                                                       d_tag.data_ptr() if with_tag else None, n)
    torch.cuda.synchronize()
    assert st == 0 and ng <= nm <= ns <= nl <= n
    start, length, index, tag = (t.cpu().numpy() for t in tensors)
    assert all(np.all(a[n:] == POISON) for a in (start, length, index, tag)), "wrote at or beyond capacity"
    assert np.array_equal(d_in[in_offset:in_offset + n].cpu().numpy(), data), "the caller's input was modified"
    assert with_index or np.all(index == POISON)
    assert with_tag or np.all(tag == POISON)
    got = (start[:ns].copy(), length[:ns].copy(), index[:ns].copy(), tag[:ns].copy(), (nl, ns, nm, ng))
    return (got, (d_in, in_offset, d_start, d_len)) if keep else got
