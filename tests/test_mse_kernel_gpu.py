"""aslp_mse_eval (csrc/nn_fused.hip), the raw entry point, against tests/mse_ref.py on both access paths.

Buffers have strides of cols rounded up to 16 with NaN in every padding float of the inputs and a sentinel in every padding float of
diff (the 16-byte path, its ragged last group included); the same matrices also sit as column windows at offsets 1 and 7 of a matrix 16
columns wider, the neighbours' inputs NaN and their outputs sentinels (the one-column path a MultiTask window takes).  Every operation
of the diff is one fp32 rounding, so it is compared bit for bit; a row's loss is a float64 sum of cols non-negative terms, whose order the
kernel is free to choose: cols * 2^-53 relative, rows * cols * 2^-53 for the batch."""
import numpy as np
import pytest
import torch

import mse_ref

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-12345.5)


def layouts(cols):
    """(name, stride, column offset): a matrix of its own, and windows at columns 1 and 7 of a matrix 16 columns wider"""
    s = (cols + 15) // 16 * 16
    return [("own", s, 0), ("window1", s + 16, 1), ("window7", s + 16, 7)]


def place(a, stride, off, fill):
    buf = np.full((a.shape[0], stride), fill, np.float32)
    buf[:, off:off + a.shape[1]] = a
    return buf


@pytest.fixture(scope="module")
def cases():
    """inputs and the model's results per shape and scale, computed once"""
    out = {}
    for rows, cols in mse_ref.SHAPES:
        y, t, w = mse_ref.inputs(rows, cols, 7000 * rows + cols)
        out[rows, cols] = (y, t, w, {sc: mse_ref.model(y, t, w, sc) for sc in (1.0, 0.25)})
    return out


@pytest.mark.parametrize("rows,cols", mse_ref.SHAPES)
def test_mse_eval_matches_model(aslp, dev, cases, rows, cols):
    y, t, w, want = cases[rows, cols]
    wd = torch.from_numpy(w).to(dev)
    for name, stride, off in layouts(cols):
        yb = torch.from_numpy(place(y, stride, off, np.nan)).to(dev)
        tb = torch.from_numpy(place(t, stride, off, np.nan)).to(dev)
        yv, tv = yb[:, off:off + cols], tb[:, off:off + cols]
        for scale in (1.0, 0.25):
            diff, row_loss, total = want[scale]
            results = []
            for call in range(2):
                db = torch.full((rows, stride), float(SENTINEL), dtype=torch.float32, device=dev)
                rl = torch.full((rows,), -1.0, dtype=torch.float64, device=dev)
                parts = torch.full((256,), -1.0, dtype=torch.float32, device=dev)
                served, nparts = aslp.ops.mse_eval(yv, tv, wd, db[:, off:off + cols], rl, scale=scale, parts=parts)
                aslp.check_error()
                assert served == 1
                results.append((db.cpu().numpy(), rl.cpu().numpy(), parts.cpu().numpy(), nparts))
            got, got_rl, got_parts, nparts = results[0]
            tag = "%s scale %g" % (name, scale)
            assert np.array_equal(got[:, off:off + cols].view(np.uint32), diff.view(np.uint32)), tag
            keep = np.ones((rows, stride), bool)
            keep[:, off:off + cols] = False
            assert (got[keep] == SENTINEL).all(), tag           # nothing written outside [rows x cols]
            err_row = np.abs(got_rl - row_loss)
            print("%s: max row-loss error / bound %.3g, total error / bound %.3g" % (
                tag, float(np.max(err_row / np.maximum(mse_ref.row_bound(cols) * row_loss, 1e-300))),
                abs(got_rl.sum() - total) / max(mse_ref.total_bound(rows, cols) * total, 1e-300)))
            assert (err_row <= mse_ref.row_bound(cols) * row_loss).all(), tag
            assert abs(float(got_rl.sum()) - total) <= mse_ref.total_bound(rows, cols) * total, tag
            assert 1 <= nparts <= 256, tag
            assert (got_parts[nparts:] == -1.0).all(), tag
            assert float(got_parts[:nparts].max()) == float(np.abs(diff).max()), tag
            # a second call: the same bits everywhere
            for a, b in zip(results[0][:3], results[1][:3]):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), tag
            assert results[1][3] == nparts


def test_non_finite_elements_do_not_set_the_maximum(aslp, dev):
    """parts hold the largest FINITE |diff| (as s16_absmax4): an inf or NaN element stays in diff and in its row's loss alone"""
    y, t, w = mse_ref.inputs(5, 9, 3)
    w[:] = 1.0
    y[1, 2], y[3, 8] = np.inf, np.nan
    diff, row_loss, _ = mse_ref.model(y, t, w)
    for stride, off in ((16, 0), (32, 7)):
        yb, tb = torch.from_numpy(place(y, stride, off, np.nan)).to(dev), torch.from_numpy(place(t, stride, off, np.nan)).to(dev)
        db = torch.zeros((5, stride), dtype=torch.float32, device=dev)
        rl = torch.zeros(5, dtype=torch.float64, device=dev)
        parts = torch.zeros(256, dtype=torch.float32, device=dev)
        served, nparts = aslp.ops.mse_eval(yb[:, off:off + 9], tb[:, off:off + 9], torch.from_numpy(w).to(dev), db[:, off:off + 9], rl, parts=parts)
        aslp.check_error()
        assert served == 1
        got = db.cpu().numpy()[:, off:off + 9]
        assert np.array_equal(got.view(np.uint32)[np.isfinite(diff)], diff.view(np.uint32)[np.isfinite(diff)])
        assert np.isinf(got[1, 2]) and np.isnan(got[3, 8])
        r = rl.cpu().numpy()
        assert np.isinf(r[1]) and np.isnan(r[3]) and np.isfinite(r[[0, 2, 4]]).all()
        assert float(parts[:nparts].max()) == float(np.abs(diff[np.isfinite(diff)]).max())


def test_device_frame_count(aslp, dev):
    """aslp_mse_eval_w: the weights summed in index order in double, truncated toward zero"""
    for w in (np.array([0.5, 2.0, 0.0], np.float32), np.full(1000, 0.7, np.float32), np.array([0.25], np.float32)):
        rows = len(w)
        y = torch.zeros((rows, 4), dtype=torch.float32, device=dev)
        d = torch.empty_like(y)
        rl = torch.empty(rows, dtype=torch.float64, device=dev)
        fr = torch.full((1,), -1.0, dtype=torch.float64, device=dev)
        served, _ = aslp.ops.mse_eval(y, y, torch.from_numpy(w).to(dev), d, rl, frames_out=fr)
        aslp.check_error()
        assert served == 1 and float(fr[0]) == mse_ref.num_frames(w)


def test_refusals(aslp, dev):
    y = torch.zeros((4, 8), dtype=torch.float32, device=dev)
    t, d = torch.zeros_like(y), torch.full_like(y, float(SENTINEL))
    w = torch.ones(4, dtype=torch.float32, device=dev)
    rl = torch.full((4,), -1.0, dtype=torch.float64, device=dev)
    for missing in range(5):
        args = [y, t, w, d, rl]
        args[missing] = None
        served, _ = aslp.ops.mse_eval(*args)
        assert served == 0
        with pytest.raises(RuntimeError, match="aslp_mse_eval"):
            aslp.check_error()
    md = aslp.MatrixDim
    import ctypes as C
    for rows, cols in ((0, 8), (4, 0), (-1, 8), (4, -3)):
        served = aslp.lib.aslp_mse_eval(aslp.ops.ptr(y), md(rows, cols, 8), aslp.ops.ptr(t), 8, aslp.ops.ptr(w), C.c_float(1.0), aslp.ops.ptr(d), 8,
                                        aslp.ops.ptr(rl), None)
        assert served == 0
        with pytest.raises(RuntimeError, match="aslp_mse_eval"):
            aslp.check_error()
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == SENTINEL).all() and (rl.cpu().numpy() == -1.0).all()   # a refusal launches nothing
