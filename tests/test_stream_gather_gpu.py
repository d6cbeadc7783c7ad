"""aslp_gather_stream_rows (csrc/stream_batch.hip): the multi-stream batch gathered on the device, bit for bit against numpy.take.
Destination row r belongs to stream r % S and receives row src_frame[r] of that stream's source, or +0.0 where src_frame[r] is -1.
Compared as uint32 bit patterns, so NaN payloads and -0.0 count; padding columns of both sides are poisoned and must come back untouched."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

POISON = np.uint32(0x7FC0BEEF)      # a NaN with a payload nobody produces
S_LIST = (1, 3, 32, 65)
B_LIST = (1, 2, 20)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32)


def from_bits(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev).view(torch.float32)


def make_case(rng, D, S, B, pad, misalign):
    """sources with their padding poisoned, a plan that holds every index pattern, and the expected bits from numpy.take"""
    ld_src = D + (12 if pad else 0)
    rows = [int(x) for x in rng.integers(1, 9, S)]
    if S > 1:
        rows[S - 1] = 0                      # a stream without rows: all of its entries are -1
    if S > 2:
        rows[1] = 1                          # row 0 is also the last row
    src_bits, plan = [], np.empty((B, S), np.int32)
    for s in range(S):
        a = rng.integers(0, 1 << 32, (rows[s], D), dtype=np.uint64).astype(np.uint32)   # any bit pattern: NaNs with payloads, denormals, infinities
        if rows[s]:
            a[0, 0] = 0x80000000             # -0.0
            a[-1, -1] = 0x7FA00001           # a signalling NaN with a payload
            a[rows[s] // 2, D // 2] = 0xFFC12345
        src_bits.append(a)
        if rows[s] == 0:
            plan[:, s] = -1
        else:
            plan[:, s] = rng.integers(-1, rows[s], B)
            plan[0, s] = 0                   # row 0 ...
            plan[-1, s] = rows[s] - 1        # ... and the last row
            if s % 4 == 2:
                plan[:, s] = rows[s] - 1     # one row repeated down a whole column of t: the delay clamp
            if s % 4 == 3:
                plan[B // 2, s] = -1
    want = np.zeros((B * S, D), np.uint32)
    flat = plan.reshape(-1)
    for r in range(B * S):
        if flat[r] >= 0:
            want[r] = np.take(src_bits[r % S], flat[r], axis=0)
    return rows, ld_src, src_bits, flat, want


def upload_sources(src_bits, D, ld_src, misalign, dev):
    """all sources in one poisoned buffer (one upload), each a view [rows x D] with row stride ld_src that starts on a 16-byte boundary, or
    one float behind one (misalign).  Returns the host image of the buffer, the device buffer and the views."""
    starts, total = [], 0
    for a in src_bits:
        starts.append(total + (1 if misalign else 0))
        total += (a.shape[0] * ld_src + 1 + 3) // 4 * 4 + 4
    host = np.full(max(total, 4), POISON, np.uint32)
    for a, st in zip(src_bits, starts):
        n = a.shape[0]
        host[st:st + n * ld_src].reshape(n, ld_src)[:, :D] = a
    buf = from_bits(host, dev)
    assert buf.data_ptr() % 16 == 0
    views = [buf[st:st + a.shape[0] * ld_src].view(a.shape[0], ld_src)[:, :D] if a.shape[0] else None for a, st in zip(src_bits, starts)]
    return host, buf, views


@pytest.mark.parametrize("pad,misalign", [(False, False), (True, False), (False, True)], ids=["dense", "padded", "misaligned"])
@pytest.mark.parametrize("D", [1, 3, 4, 43, 440])
def test_gather_bits_match_numpy_take(aslp, dev, D, pad, misalign):
    rng = np.random.default_rng(1000 * D + 10 * pad + misalign)
    import ctypes as C
    StreamSrc = aslp._lib.StreamSrc
    for S in S_LIST:
        for B in B_LIST:
            rows, ld_src, src_bits, plan, want = make_case(rng, D, S, B, pad, misalign)
            host_img, buf, views = upload_sources(src_bits, D, ld_src, misalign, dev)
            ld_dst = D + (20 if pad else 0)
            dst_buf = from_bits(np.full(B * S * ld_dst, POISON, np.uint32), dev).view(B * S, ld_dst)
            dst = dst_buf[:, :D]
            # the path the launcher takes is the one this case is meant for
            table = (StreamSrc * S)()
            for s, v in enumerate(views):
                if v is not None:
                    table[s].base, table[s].stride, table[s].rows = v.data_ptr(), ld_src, rows[s]
            vec = aslp.lib.aslp_gather_stream_rows_path(C.c_void_p(dst.data_ptr()), ld_dst, S, D, table)
            live = any(r > 0 for r in rows)
            assert vec == int(D % 4 == 0 and (not misalign or not live)), (D, S, B, vec)
            for again in range(2):           # a second call gives the same bits
                aslp.ops.gather_stream_rows(dst, views, plan)
                got = bits(dst_buf)
                assert np.array_equal(got[:, :D], want), (D, S, B, again)
                assert (got[:, D:] == POISON).all(), "destination padding written"
            assert np.array_equal(bits(buf), host_img), "a source or its padding was written"


def test_minus_one_rows_are_plus_zero_and_special_values_survive(aslp, dev):
    D, S, B = 8, 2, 3
    src = np.array([[0x80000000, 0x7FA00001, 0xFFC12345, 0x00000001, 0x7F800000, 0xFF800000, 0x3F800000, 0x80000001]], np.uint32)
    a = from_bits(src, dev).view(1, D)
    dst = from_bits(np.full((B * S, D), POISON, np.uint32), dev).view(B * S, D)
    aslp.ops.gather_stream_rows(dst, [a, None], [0, -1, -1, -1, 0, -1])
    got = bits(dst)
    assert np.array_equal(got[0], src[0]) and np.array_equal(got[4], src[0])
    assert (got[[1, 2, 3, 5]] == 0).all()    # +0.0, not -0.0 and not what was there


def test_out_of_range_index_is_refused_without_a_launch(aslp, dev):
    D, S, B = 4, 3, 2
    srcs = [torch.ones(n, D, device=dev) for n in (2, 5, 1)]
    dst = from_bits(np.full((B * S, D), POISON, np.uint32), dev).view(B * S, D)
    for bad in ([0, 0, 0, 2, 0, 0], [0, 5, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0], [-2, 0, 0, 0, 0, 0]):
        with pytest.raises(RuntimeError, match="aslp_gather_stream_rows"):
            aslp.ops.gather_stream_rows(dst, srcs, bad)
        assert (bits(dst) == POISON).all(), "a refused plan must not launch"
    with pytest.raises(RuntimeError, match="aslp_gather_stream_rows"):   # an entry for a stream without rows
        aslp.ops.gather_stream_rows(dst, [srcs[0], None, srcs[2]], [0, 0, 0, 0, -1, 0])
    assert (bits(dst) == POISON).all()
    aslp.ops.gather_stream_rows(dst, srcs, [1, 4, 0, -1, 0, 0])           # the library is usable afterwards
    assert np.array_equal(bits(dst)[:3], bits(torch.ones(3, D)))
