"""aslp_xent_blocks_eval (csrc/nn_fused.hip), the raw entry point: Xent over column blocks of one matrix in one launch.

Every operand sits in a buffer wider than the matrix (stride > cols, the matrix at column `base`): NaN in every float of the activations
that belongs to no block, a sentinel in every such float of diff and post_out, checked afterwards.  Against the code that exists: the
posteriors are cudaF_softmax_reduce's on the same window bit for bit, the unmasked diff is aslp_xent_eval's (labels) on those posteriors
times the task weight in fp32 bit for bit, frames and correct are exact and the three other sums hold rtol 1e-5 / atol 1e-6
(tests/test_bn_xent_kernels_gpu.py's bar for xent_rows_kernel).  The masked diff holds 1e-4 relative l2 per block against
tests/multitask_ref.py (the mask's factor 1 - s carries the rounding of an fp32 sum over the block's row)."""
import numpy as np
import pytest
import torch

import multitask_ref as ref

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-12345.5)


def stride_of(case):
    return (ref.total_cols(case) + case.base + 3) // 4 * 4 + 4


def place(a, stride, base, fill):
    buf = np.full((a.shape[0], stride), fill, np.float32)
    buf[:, base:base + a.shape[1]] = a
    return buf


@pytest.fixture(scope="module")
def references(aslp, dev):
    """per case, computed once with the kernels that exist: the window's posteriors, the per-block diff and sums on them"""
    out = {}
    for case in ref.CASES:
        acts, labels, fw, weights = ref.inputs(case)
        rows, total, stride, base = case.rows, ref.total_cols(case), stride_of(case), case.base
        blocks = list(zip(ref.offsets_of(case), case.widths))
        ab = torch.from_numpy(place(acts, stride, base, np.nan)).to(dev)
        pb = torch.full((rows, stride), float(SENTINEL), dtype=torch.float32, device=dev)
        fwd = torch.from_numpy(fw).to(dev)
        diff = np.zeros((rows, total), np.float32)
        sums = []
        for b, (off, cols) in enumerate(blocks):
            win = slice(base + off, base + off + cols)
            aslp.ops.softmax(pb[:, win], ab[:, win])
            d = torch.empty((rows, cols), dtype=torch.float32, device=dev)
            st = torch.zeros(5, dtype=torch.float64, device=dev)
            aslp.ops.xent_eval(pb[:, win], fwd, d, st, labels=torch.from_numpy(np.ascontiguousarray(labels[:, b])).to(dev))
            if weights[b] != 1.0:
                d = d * np.float32(weights[b])
            diff[:, off:off + cols] = d.cpu().numpy()
            sums.append(st.cpu().numpy())
        aslp.check_error()
        out[case.name] = dict(acts=acts, labels=labels, fw=fw, weights=weights, blocks=blocks, post=pb.cpu().numpy(), diff=diff, sums=sums)
    return out


def run(aslp, dev, case, r, inp, softmax, mask):
    """one call on fresh sentinel-filled outputs; everything it left, on the host"""
    rows, stride, base, total = case.rows, stride_of(case), case.base, ref.total_cols(case)
    ib = torch.from_numpy(inp).to(dev)
    db = torch.full((rows, stride), float(SENTINEL), dtype=torch.float32, device=dev)
    pb = torch.full((rows, stride), float(SENTINEL), dtype=torch.float32, device=dev)
    rs = [torch.full((rows, 5), -7.0, dtype=torch.float64, device=dev) for _ in r["blocks"]]
    parts = torch.full((256,), -1.0, dtype=torch.float32, device=dev)
    blocks = [(off, cols, w, t) for (off, cols), w, t in zip(r["blocks"], r["weights"], rs)]
    win = slice(base, base + total)
    served, nparts = aslp.ops.xent_blocks_eval(ib[:, win], blocks, torch.from_numpy(r["labels"]).to(dev), torch.from_numpy(r["fw"]).to(dev),
                                               db[:, win], softmax=softmax, mask=mask, post_out=pb[:, win], parts=parts)
    aslp.check_error()
    assert served == 1
    sums = []
    for t in rs:
        st = torch.zeros(5, dtype=torch.float64, device=dev)
        aslp.ops.xent_sum_rowstats(t, rows, 1, st)
        sums.append(st.cpu().numpy())
    aslp.check_error()
    return dict(diff=db.cpu().numpy(), post=pb.cpu().numpy(), rowstats=[t.cpu().numpy() for t in rs], sums=sums, parts=parts.cpu().numpy(), nparts=nparts)


def covered(case, r):
    m = np.zeros((case.rows, stride_of(case)), bool)
    for off, cols in r["blocks"]:
        m[:, case.base + off:case.base + off + cols] = True
    return m


@pytest.mark.parametrize("softmax", [1, 0])
@pytest.mark.parametrize("name", ref.CASE_NAMES)
def test_bits_of_the_existing_kernels(aslp, dev, references, name, softmax):
    """mask = 0: posteriors, diff and sums against cudaF_softmax_reduce, aslp_xent_eval and the task weight's fp32 product"""
    case, r = ref.CASES[ref.CASE_NAMES.index(name)], references[name]
    stride, base, total = stride_of(case), case.base, ref.total_cols(case)
    m = covered(case, r)
    # softmax = 0: `in` holds the posteriors (NaN wherever no block lies)
    inp = place(r["acts"], stride, base, np.nan) if softmax else np.where(m, r["post"], np.float32(np.nan)).astype(np.float32)
    a, b = run(aslp, dev, case, r, inp, softmax, 0), run(aslp, dev, case, r, inp, softmax, 0)
    assert np.array_equal(a["post"][m].view(np.uint32), r["post"][m].view(np.uint32))
    assert (a["post"][~m] == SENTINEL).all() and (a["diff"][~m] == SENTINEL).all()   # padding and the columns of no block
    got = a["diff"][:, base:base + total]
    for k, (off, cols) in enumerate(r["blocks"]):
        assert np.array_equal(got[:, off:off + cols].view(np.uint32), r["diff"][:, off:off + cols].view(np.uint32)), (name, k)
        s, w = a["sums"][k], r["sums"][k]
        print("%s block %d: sums %s against %s" % (name, k, s, w))
        assert s[0] == w[0] and s[1] == w[1], (name, k)
        assert np.allclose(s[2:], w[2:], rtol=1e-5, atol=1e-6), (name, k)
    # the float64 model agrees with what the existing kernels gave (the inputs' arg-max gap makes `correct` exact)
    _, stats = ref.model(r["post"][:, base:base + total], r["blocks"], r["weights"], r["labels"], r["fw"], mask=False)
    for k, st in enumerate(stats):
        assert a["sums"][k][0] == st["frames"] and a["sums"][k][1] == st["correct"], (name, k)
        assert np.allclose(a["sums"][k][2:], [st["loss"], st["entropy"], st["likelyhood"]], rtol=1e-5, atol=1e-6), (name, k)
    # per-workgroup maxima: workgroup b of the nparts = min(rows, 256) serves rows b, b + nparts, ...
    nparts = a["nparts"]
    assert nparts == min(case.rows, 256) and (a["parts"][nparts:] == -1.0).all()
    dmax = torch.from_numpy(np.where(m, a["diff"], np.float32(0))).abs().amax(dim=1).numpy()
    for wg in range(nparts):
        assert a["parts"][wg] == dmax[wg::nparts].max(), (name, wg)
    # a second call: the same bits everywhere
    for key in ("diff", "post", "parts"):
        assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), (name, key)
    for x, y in zip(a["rowstats"], b["rowstats"]):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), name


@pytest.mark.parametrize("softmax", [1, 0])
@pytest.mark.parametrize("name", ref.CASE_NAMES)
def test_masked_diff_against_float64(aslp, dev, references, name, softmax):
    case, r = ref.CASES[ref.CASE_NAMES.index(name)], references[name]
    stride, base, total = stride_of(case), case.base, ref.total_cols(case)
    m = covered(case, r)
    inp = place(r["acts"], stride, base, np.nan) if softmax else np.where(m, r["post"], np.float32(np.nan)).astype(np.float32)
    a, b = run(aslp, dev, case, r, inp, softmax, 1), run(aslp, dev, case, r, inp, softmax, 1)
    want, _ = ref.model(r["post"][:, base:base + total], r["blocks"], r["weights"], r["labels"], r["fw"], mask=True)
    got = a["diff"][:, base:base + total]
    for k, (off, cols) in enumerate(r["blocks"]):
        err = ref.rel_l2(got[:, off:off + cols], want[:, off:off + cols])
        print("%s block %d: masked diff rel l2 %.3g" % (name, k, err))
        assert err <= 1e-4, (name, k)
    assert (a["diff"][~m] == SENTINEL).all() and (a["post"][~m] == SENTINEL).all()
    assert np.array_equal(a["post"][m].view(np.uint32), r["post"][m].view(np.uint32))
    for k in range(len(r["blocks"])):   # the mask touches the diff alone
        assert a["sums"][k][0] == r["sums"][k][0] and a["sums"][k][1] == r["sums"][k][1], (name, k)
        assert np.allclose(a["sums"][k][2:], r["sums"][k][2:], rtol=1e-5, atol=1e-6), (name, k)
    for key in ("diff", "post", "parts"):
        assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), (name, key)


@pytest.mark.parametrize("name", ["wave_slot_edge", "medium_aligned", "medium_offset3"])
def test_mask_on_rows_that_do_not_sum_to_one(aslp, dev, references, name):
    """softmax = 0 on posteriors x 1.25: the block's diff row sums to 0.25 x frame weight x task weight, the mask's factor 1 - s is 0.5 ..
    0.94, far from 1 -- a kernel that leaves the mask out misses the bar by orders of magnitude.  (Not x 1.5: with frame weight 2 and task
    weight 1 the row sum is 1 and the factor a difference of two equal numbers, which no fp32 sum holds to 1e-4.)"""
    case, r = ref.CASES[ref.CASE_NAMES.index(name)], references[name]
    stride, base, total = stride_of(case), case.base, ref.total_cols(case)
    m = covered(case, r)
    inp = np.where(m, r["post"] * np.float32(1.25), np.float32(np.nan)).astype(np.float32)
    a = run(aslp, dev, case, r, inp, 0, 1)
    y = inp[:, base:base + total]
    want, _ = ref.model(y, r["blocks"], r["weights"], r["labels"], r["fw"], mask=True)
    plain, _ = ref.model(y, r["blocks"], r["weights"], r["labels"], r["fw"], mask=False)
    got = a["diff"][:, base:base + total]
    live = 0
    for k, (off, cols) in enumerate(r["blocks"]):
        err = ref.rel_l2(got[:, off:off + cols], want[:, off:off + cols])
        print("%s block %d: rel l2 %.3g (unmasked model: %.3g)" % (name, k, err, ref.rel_l2(plain[:, off:off + cols], want[:, off:off + cols])))
        assert err <= 1e-4, (name, k)
        live += ref.rel_l2(plain[:, off:off + cols], want[:, off:off + cols]) > 0.05
    assert live >= 1   # (the case does tell the two apart)
    assert np.array_equal(a["post"][m].view(np.uint32), inp[m].view(np.uint32))   # post_out: what `in` held


def test_refusals(aslp, dev):
    rows, cols = 4, 24
    x = torch.zeros((rows, cols), dtype=torch.float32, device=dev)
    d, p = torch.full_like(x, float(SENTINEL)), torch.full_like(x, float(SENTINEL))
    w = torch.ones(rows, dtype=torch.float32, device=dev)
    rs = torch.full((rows, 5), -1.0, dtype=torch.float64, device=dev)
    lab = torch.zeros((rows, 17), dtype=torch.int32, device=dev)
    wide = torch.zeros((rows, 8200), dtype=torch.float32, device=dev)
    dwide = torch.full_like(wide, float(SENTINEL))
    for what, args in (("17 blocks", (x, [(k, 1, 1.0, rs) for k in range(17)], lab, w, d)),
                       ("overlap", (x, [(0, 10, 1.0, rs), (9, 5, 1.0, rs)], lab, w, d)),
                       ("outside", (x, [(20, 5, 1.0, rs)], lab, w, d)),
                       ("8193", (wide, [(0, 8193, 1.0, rs)], lab, w, dwide)),
                       ("null diff", (x, [(0, 10, 1.0, rs)], lab, w, None)),
                       ("no blocks", (x, [], lab, w, d)),
                       ("null rowstats", (x, [(0, 10, 1.0, None)], lab, w, d))):
        served, _ = aslp.ops.xent_blocks_eval(*args, post_out=p if args[0] is x else None)
        assert served == 0, what
        with pytest.raises(RuntimeError, match="aslp_xent_blocks_eval"):
            aslp.check_error()
    torch.cuda.synchronize()
    for t, v in ((d, SENTINEL), (p, SENTINEL), (dwide, SENTINEL), (rs, -1.0)):
        assert (t.cpu().numpy() == v).all()   # a refusal launches nothing
    assert aslp.lib.aslp_xent_blocks_supported(1) == 1 and aslp.lib.aslp_xent_blocks_supported(8192) == 1
    assert aslp.lib.aslp_xent_blocks_supported(0) == 0 and aslp.lib.aslp_xent_blocks_supported(8193) == 0
