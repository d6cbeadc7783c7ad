"""Ten small, in-bounds changes to the substrate kernels (csrc/ew_kernels.hip, conv_pool.hip, reduce_kernels.hip, optim_kernels.hip): does
tests/test_substrate_kernels_gpu.py notice each?  Every change alters arithmetic or reads fewer elements; none moves an access out of bounds.

    python devtools/substrate_mutations.py            # edit the sources in place
    make -C kaldi-aslp_amd && pytest tests/test_substrate_kernels_gpu.py
    python devtools/substrate_mutations.py --revert   # put them back, then make again

On an MI355X the changed library failed 53 of the file's tests, each change at least one (the test file's docstring lists them)."""
import os
import sys

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kaldi-aslp_amd", "csrc")
CHANGES = [
    # map_vec4's second lane passes column c for c + 1: a row vector is read one element early
    ("ew_kernels.hip", "o.y = f(d.y, av.y, bv.y, r, c + 1);", "o.y = f(d.y, av.y, bv.y, r, c);"),
    # add_rows' fourth lane adds the third element
    ("ew_kernels.hip", "o.w += alpha * v.w;", "o.w += alpha * v.z;"),
    # conv in-diff: the last of several patches is dropped
    ("conv_pool.hip", "for (int p = p_lo; p <= p_hi; p++) acc +=", "for (int p = p_lo; p < p_hi + (p_lo == p_hi); p++) acc +="),
    # max-pool forward: another reset value
    ("conv_pool.hip", "float m = -1e20f;   // :110", "float m = -1e30f;   // :110"),
    # add_col_sum_mat_vec: the last column of a row wider than 64 is dropped
    ("reduce_kernels.hip", "for (int c = lane; c < d.cols; c += 64) s += row[c];\n    s = wave_sum(s);\n    if (lane == 0) v[r] = beta",
     "for (int c = lane; c < d.cols - (d.cols > 64); c += 64) s += row[c];\n    s = wave_sum(s);\n    if (lane == 0) v[r] = beta"),
    # Adam without its second bias correction
    ("optim_kernels.hip", "inv_sqrt_floor(v * a.corr2)", "inv_sqrt_floor(v)"),
    # d2f truncates
    ("ew_kernels.hip", "dst[i] = (float)src[i];", "dst[i] = __double2float_rz(src[i]);"),
    # group p-norm: the rescale branch is never taken
    ("conv_pool.hip", "if (t == HUGE_VALF) ok = false;", "if (t == HUGE_VALF) ok = true;"),
    # scatter_add ignores column 0
    ("ew_kernels.hip", "c >= 0 && c < d.cols) atomicAdd", "c > 0 && c < d.cols) atomicAdd"),
    # splice backward clamps one row early at the end
    ("ew_kernels.hip", "sr = sr < 0 ? 0 : (sr >= rows ? rows - 1 : sr);\n      const float *p = od", "sr = sr < 0 ? 0 : (sr >= rows ? rows - 2 : sr);\n      const float *p = od"),
]


def main():
    revert = "--revert" in sys.argv[1:]
    for name, old, new in CHANGES:
        if revert:
            old, new = new, old
        path = os.path.join(CSRC, name)
        text = open(path).read()
        if text.count(old) != 1:
            sys.exit("%s: expected exactly one occurrence of %r" % (name, old))
        open(path, "w").write(text.replace(old, new))
    print("%s %d changes" % ("reverted" if revert else "applied", len(CHANGES)))


if __name__ == "__main__":
    main()
