"""Single launches of the classifier head's exact-fp32 GEMM and small training kernels against references, element by element.

Each harness call (cbas_debug_head_run, debug build) feeds host operands to ONE launcher of gemm_f32.hip /
head_train_kernels.hip.  The references are oracle/kernel_ref.py's (validated on the CPU by
tests/test_kernel_reference_bounds.py):
  - bit for bit: the GEMM without GELU (the fmaf chain in the MFMA's k order, one fp32 bias addition; split-K partials and
    their z-ascending sum), transpose_pad, add_vec / copy, sub_colmean, cov_offdiag's G, colsum (tmp and dst, in the
    kernel's chunk order);
  - bounded per element from where the kernel rounds: the fused GELU, colsum against the float64 sum, cov_offdiag's sq,
    ce_terms / ce_grad, gelu_dropout (whose keep mask and exact zeros must also match the oracle's hash), adam (p, m, v).
Everything a launch does not own - rows past M, columns N .. ldo, the floats past an image's last element - is the caller's
canary and must come back unchanged; NaN sits in every operand element a launch must not use.  Every `_multi` launcher runs
k = 1, 3, 8 entries of unequal size (one empty, the largest not first): each entry equals the single-trial launcher's
output bit for bit and meets the same reference.  The harness refuses, by return code and without launching, every shape a
launcher would mis-handle.  Each test prints its largest max |error| / bound (run with -s)."""
import ctypes as C

import numpy as np
import pytest

from cbas_amd import _lib
from oracle import kernel_ref as R

pytestmark = pytest.mark.gpu

c_int, c_int64, c_uint64, c_uint32, c_float, c_void_p = C.c_int, C.c_int64, C.c_uint64, C.c_uint32, C.c_float, C.c_void_p
(GEMM, TRANSPOSE_PAD, GELU_FWD, GELU_BWD, CE_TERMS, CE_GRAD, COV_OFFDIAG, SUB_COLMEAN, COLSUM, ADD_VEC, ADAM) = range(11)
EINVAL = -1
CANARY = np.float32(-31337.25)
TAIL = 5                                   # canary floats past every output image
F32 = np.float32


class Entry(C.Structure):                  # include/cbas_mi355x_debug.h cbas_debug_head_entry
    _fields_ = ([(n, c_int64) for n in ("n", "rows_pad", "ld", "wd_lo", "wd_hi")] + [("key", c_uint64)] +
                [(n, c_int) for n in ("cols", "C", "step")] + [("thr", c_uint32)] +
                [(n, c_float) for n in ("eps", "scale", "cscale", "gscale", "lr", "wd", "wd_special")] +
                [("in_", c_void_p * 4), ("in_bytes", c_int64 * 4), ("out", c_void_p * 3), ("out_bytes", c_int64 * 3)])


class HeadArgs(C.Structure):               # cbas_debug_head_args
    _fields_ = ([("struct_bytes", c_int64), ("entry_bytes", c_int64)] +
                [(n, c_int) for n in ("op", "multi", "k", "gelu", "splits", "N", "N_alloc", "K")] +
                [(n, c_int64) for n in ("M", "lda", "ldw", "ldo", "split_stride")] + [("entries", c_void_p)])


def entry(ins=(), outs=(), **kw):
    """(Entry fields, input arrays, output arrays): inputs may be None (an absent optional operand)."""
    return dict(kw), list(ins), list(outs)


def head_call(op, entries, *, multi=0, in_bytes=None, out_bytes=None, **top):
    """One harness call; returns its code.  Output arrays are updated in place.  in_bytes / out_bytes: {(entry, slot): bytes}
    claims that differ from the arrays' sizes (the refusal tests)."""
    lib = _lib.load()
    arr = (Entry * len(entries))()
    keep = []
    for j, (kw, ins, outs) in enumerate(entries):
        for name, v in kw.items():
            setattr(arr[j], name, v)
        for i, t in enumerate(ins):
            if t is None:
                continue
            t = np.ascontiguousarray(t)
            keep.append(t)
            arr[j].in_[i] = t.ctypes.data if t.size else None
            arr[j].in_bytes[i] = (in_bytes or {}).get((j, i), t.nbytes)
        for i, t in enumerate(outs):
            assert t.flags.c_contiguous
            arr[j].out[i] = t.ctypes.data if t.size else None
            arr[j].out_bytes[i] = (out_bytes or {}).get((j, i), t.nbytes)
    a = HeadArgs()
    a.struct_bytes, a.entry_bytes = C.sizeof(HeadArgs), C.sizeof(Entry)
    a.op, a.multi, a.k = op, multi, top.pop("k", len(entries))
    for name, v in top.items():
        setattr(a, name, v)
    a.entries = C.addressof(arr)
    return lib.cbas_debug_head_run(C.byref(a))


def run(op, entries, **kw):
    _lib.check(head_call(op, entries, **kw), f"cbas_debug_head_run(op {op})")


def image(n, fill=CANARY):
    """An output image of n floats followed by TAIL canaries."""
    return np.full(int(n) + TAIL, fill, F32)


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- GEMM ---------------------------------------------------------------------------------------------------------------
GEMM_N = [4, 12, 128, 132, 260]
GEMM_K = [32, 64, 96, 768]


def gemm_run(A, W, b, *, M, N, K, N_alloc, lda, ldw, ldo, gelu, rows_extra=2):
    out = np.full((M + rows_extra, ldo), CANARY, F32)
    run(GEMM, [entry([A, W, b], [out])], M=M, N=N, N_alloc=N_alloc, K=K, lda=lda, ldw=ldw, ldo=ldo, gelu=gelu)
    return out


GEMM_M = [1, 127, 128, 129, 257]


@pytest.mark.parametrize("M", GEMM_M)
def test_gemm_is_the_fmaf_chain_bit_for_bit_and_gelu_within_bound(M):
    """Every M with every N and K = 32, 64, 96.  The long chain K = 768 (the reference's cost) runs on every other N,
    alternating with the index of M: N = 4, 128, 260 meet it at M = 1, 128, 257 and N = 12, 132 at M = 127, 129, so every N
    meets it on both sides of a tile edge; (M = 127 / 129, N = 4 / 128 / 260, K = 768) and (M = 1 / 128 / 257, N = 12 / 132,
    K = 768) are not run.  The N_alloc, lda, ldo, bias and NaN-row choices rotate over the grid, they are not crossed: each
    choice meets each M, N and K, not each combination of them."""
    worst = 0.0
    mi = GEMM_M.index(M)
    for ni, N in enumerate(GEMM_N):
        for ki, K in enumerate(GEMM_K):
            c = ni + ki + M                                          # rotates the options over the (N, K) grid
            if K == 768 and (ni + mi) % 2:                           # the long chain on every other N: the reference's cost
                continue
            N_alloc = N + 4 * (c % 2)
            lda = K + 4 * ((c // 2) % 2)
            ldo = N + 8 * ((c // 4 + ni) % 2)
            bias = (c // 3) % 2 == 0
            nan_row = M // 2 if M > 1 and c % 3 == 0 else None
            A, W, b = R.head_gemm_case(M, N, K, 1000 * M + 10 * N + K, N_alloc=N_alloc, lda=lda, bias=bias, nan_row=nan_row)
            pre, _ = R.head_gemm_exact(A[:, :K], W[:N, :K], b, K)
            clean = np.ones(M, bool)
            if nan_row is not None:
                clean[nan_row] = False
            for gelu in (0, 1):
                out = gemm_run(A, W, b, M=M, N=N, K=K, N_alloc=N_alloc, lda=lda, ldw=0, ldo=ldo, gelu=gelu)
                tag = (M, N, K, N_alloc, lda, ldo, bias, gelu)
                assert (out[M:] == CANARY).all() and (out[:, N:] == CANARY).all(), ("canary changed", tag)
                got = out[:M, :N]
                assert np.isnan(got[~clean]).all(), ("a NaN row of A must give a NaN row", tag)
                assert np.isfinite(got[clean]).all(), ("NaN left its row / an unread operand was used", tag)
                if not gelu:
                    assert same_bits(got[clean], pre[clean]), ("not the fmaf chain + one bias addition", tag)
                else:
                    y, bound = R.head_gemm_gelu_ref(pre[clean])
                    r = R.ratio(got[clean], y, bound)
                    worst = max(worst, r)
                    assert r <= 1.0, (tag, r)
    print(f"[head gemm M {M}] plain: bit for bit; GELU max err / bound {worst:.3f}")


@pytest.mark.parametrize("M,N", [(12, 128), (129, 36)])
def test_gemm_split_k_partials_and_sum_bit_for_bit(M, N):
    for Kt, splits in ((1024, 2), (1024, 4), (2048, 4), (2048, 16), (8192, 16), (8192, 2)):
        K = Kt // splits
        stride = M * N + (8 if (Kt, splits) == (2048, 4) else 0)                  # one case with split_stride > M N
        A, W, _ = R.head_gemm_case(M, N, Kt, Kt + splits + M, bias=False)
        want, parts = R.head_gemm_exact(A, W, None, K, splits)
        out = image(M * N)
        part = image(splits * stride)
        run(GEMM, [entry([A, W, None], [out, part])], M=M, N=N, N_alloc=N, K=K, lda=Kt, ldw=Kt, ldo=N, splits=splits, split_stride=stride)
        tag = (M, N, Kt, splits, stride)
        assert (out[M * N:] == CANARY).all() and (part[splits * stride:] == CANARY).all(), ("canary past the images", tag)
        p = part[:splits * stride].reshape(splits, stride)
        assert (p[:, M * N:] == CANARY).all(), ("canary between the partials", tag)
        for z in range(splits):
            assert same_bits(p[z, :M * N].reshape(M, N), parts[z]), ("partial", z, tag)
        assert same_bits(out[:M * N].reshape(M, N), want), ("sum of the partials, z ascending", tag)
    print(f"[head gemm split-K M {M} N {N}] partials and result: bit for bit")


# ---- bit-exact small kernels -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 31, 32, 33, 100])
def test_transpose_pad(rows):
    rng = np.random.default_rng(rows)
    for cols in (1, 32, 33, 260):
        for ld in (cols, cols + 3):
            for rows_pad in (rows, rows + 1, -(-rows // 512) * 512):
                src = np.full((rows, ld), np.nan, F32)
                src[:, :cols] = rng.standard_normal((rows, cols)).astype(F32)
                dst = image(cols * rows_pad)
                run(TRANSPOSE_PAD, [entry([src], [dst], n=rows, cols=cols, ld=ld, rows_pad=rows_pad)])
                assert (dst[cols * rows_pad:] == CANARY).all(), (cols, ld, rows_pad)
                assert same_bits(dst[:cols * rows_pad].reshape(cols, rows_pad), R.transpose_pad_ref(src, rows, cols, rows_pad)), \
                    ("transpose / zero padding", cols, ld, rows_pad)
    print(f"[head transpose_pad rows {rows}] bit for bit")


SIZES = [1, 255, 256, 257, 1000]


def vec_entries(sizes, seed):
    rng = np.random.default_rng(seed)
    out = []
    for j, n in enumerate(sizes):
        a = rng.standard_normal(n).astype(F32)
        b = rng.standard_normal(n).astype(F32) if j % 2 == 0 else None          # NULL: copy
        out.append((a, b))
    return out


def test_add_vec_and_copy():
    for n in SIZES:
        for (a, b) in vec_entries([n, n], n):
            o = image(n)
            run(ADD_VEC, [entry([a, b], [o], n=n)])
            assert (o[n:] == CANARY).all() and same_bits(o[:n], a + b if b is not None else a), n
    print("[head add_vec] bit for bit")


def test_sub_colmean():
    rng = np.random.default_rng(3)
    for rows, cols in ((1, 1), (5, 51), (16, 16), (257, 1), (8, 125)):            # 1, 255, 256, 257, 1000 elements
        src = (rng.standard_normal((rows, cols)) + 3.0).astype(F32)
        cs = src.sum(0, dtype=F32)
        dst = image(rows * cols)
        run(SUB_COLMEAN, [entry([src, cs], [dst], n=rows, cols=cols)])
        assert (dst[rows * cols:] == CANARY).all() and same_bits(dst[:rows * cols].reshape(rows, cols), R.sub_colmean_f32(src, cs)), (rows, cols)
    print("[head sub_colmean] bit for bit")


colsum_case = R.colsum_case


def check_colsum(src, rows, cols, scale, tmp, dst, tag):
    t, d = R.colsum_f32(src[:, :cols], scale)
    assert (tmp[64 * cols:] == CANARY).all() and (dst[cols:] == CANARY).all(), ("canary", tag)
    assert same_bits(tmp[:64 * cols].reshape(64, cols), t), ("tmp: the chunk sums", tag)
    assert same_bits(dst[:cols], d), ("dst: chunks in order, times scale", tag)
    ref, bound = R.colsum_ref(src[:, :cols], scale)
    return R.ratio(dst[:cols], ref, bound)


@pytest.mark.parametrize("rows", [1, 37, 63, 64, 65, 1000])
def test_colsum(rows):
    worst = 0.0
    for cols in (1, 63, 64, 65, 200):
        src, ld = colsum_case(rows, cols, 7 * rows + cols)
        for scale in (1.0, 1.0 / 37.0):
            tmp, dst = image(64 * cols), image(cols)
            run(COLSUM, [entry([src], [tmp, dst], n=rows, cols=cols, ld=ld, scale=scale)])
            r = check_colsum(src, rows, cols, scale, tmp, dst, (rows, cols, scale))
            worst = max(worst, r)
            assert r <= 1.0, (rows, cols, scale, r)
    print(f"[head colsum rows {rows}] kernel order: bit for bit; vs float64 max err / bound {worst:.3f}")


cov_case = R.cov_case


def check_cov(cov, n, cs, gs, G, sq, tag):
    assert (G[n * n:] == CANARY).all() and (sq[n:] == CANARY).all(), ("canary", tag)
    g = G[:n * n].reshape(n, n)
    assert same_bits(g, R.cov_offdiag_f32(cov, cs, gs)), ("G = gscale (cov cscale)", tag)
    assert (bits(np.diagonal(g)) == 0).all(), ("diagonal must be +0", tag)
    ref, bound = R.cov_sq_ref(cov, cs)
    return R.ratio(sq[:n], ref, bound)


@pytest.mark.parametrize("n", [32, 64, 96, 100, 256])
def test_cov_offdiag(n):
    cov, cs, gs = cov_case(n, n)
    G, sq = image(n * n), image(n)
    run(COV_OFFDIAG, [entry([cov], [G, sq], n=n, cscale=cs, gscale=gs)])
    r = check_cov(cov, n, cs, gs, G, sq, n)
    assert r <= 1.0, (n, r)
    print(f"[head cov_offdiag n {n}] G: bit for bit; sq max err / bound {r:.3f}")


# ---- cross entropy --------------------------------------------------------------------------------------------------
CE_N = [1, 127, 128, 129, 1000]
CE_C = [2, 9, 12, 64]


def ce_sums(z, y, cw, eps):
    t, _ = R.ce_terms_ref(z, y, cw, eps)
    return t.sum(0).astype(F32)


def check_ce(op, z, y, cw, eps, sums, out, tag):
    n, Cc = z.shape
    size = n * (2 if op == CE_TERMS else Cc)
    assert (out[size:] == CANARY).all(), ("canary", tag)
    if op == CE_TERMS:
        ref, bound = R.ce_terms_ref(z, y, cw, eps)
        got = out[:size].reshape(n, 2)
        assert same_bits(got[:, 1], ref[:, 1]), ("w[y] is a copy", tag)
        return R.ratio(got[:, 0], ref[:, 0], bound[:, 0])
    ref, bound = R.ce_grad_ref(z, y, cw, eps, sums)
    return R.ratio(out[:size].reshape(n, Cc), ref, bound)


def libm_figure_ce(op, z, y, out):
    """What the math library adds beyond the roundings ce_terms_ref / ce_grad_ref itemise, in the unit CE_LSE_U / CE_P_U
    multiplies (kernel_ref.py): the figure those budgets were set from.  With cw NULL, eps 0 and sums[1] = 1 every product by
    1 is exact and the kernels store fl(lse - z_y) resp. fl(p - [c = y]).  The reference here takes the fp32 argument z - mx
    expf receives (its rounding is the |z - mx| term of the bound, not expf's); from the error the itemised terms are taken off:
    u32 (|lse| + |lse - z_y| + C) resp. u32 p (C + 2)."""
    zz = z.astype(np.float64)
    n, Cc = z.shape
    mx = zz.max(1, keepdims=True)
    arg = (z - z.max(1, keepdims=True)).astype(np.float64)
    den = np.exp(arg).sum(1, keepdims=True)
    if op == CE_TERMS:
        lse = (mx + np.log(den))[:, 0]
        a = lse - zz[np.arange(n), y]
        err = np.abs(out[:2 * n].reshape(n, 2)[:, 0].astype(np.float64) - a)
        excess = np.maximum(err - R.U32 * (np.abs(lse) + np.abs(a) + Cc), 0.0)
        return float((excess / (R.U32 * (1.0 + np.abs(np.log(den[:, 0]))))).max())
    p = np.exp(arg) / den
    got = out[:n * Cc].reshape(n, Cc).astype(np.float64)
    off = np.ones_like(p, bool)
    off[np.arange(n), y] = False
    off &= p > 2.0 ** -100
    excess = np.maximum(np.abs(got - p) - R.U32 * p * (Cc + 2), 0.0)
    return float((excess[off] / (R.U32 * p[off])).max()) if off.any() else 0.0


@pytest.mark.parametrize("op", [CE_TERMS, CE_GRAD], ids=["terms", "grad"])
@pytest.mark.parametrize("Cc", CE_C)
def test_cross_entropy(op, Cc):
    worst, fig = 0.0, 0.0
    for n in CE_N:
        for with_cw in (False, True):
            for eps in (0.0, 0.1):
                z, y, cw = R.ce_case(n, Cc, 100 * n + Cc, with_cw)
                sums = ce_sums(z, y, cw, eps)
                out = image(n * (2 if op == CE_TERMS else Cc))
                run(op, [entry([z, y, cw, sums], [out], n=n, C=Cc, eps=eps)])
                r = check_ce(op, z, y, cw, eps, sums, out, (n, Cc, with_cw, eps))
                worst = max(worst, r)
                assert r <= 1.0, (n, Cc, with_cw, eps, r)
        z, y, _ = R.ce_case(n, Cc, 100 * n + Cc, False)
        out = image(n * (2 if op == CE_TERMS else Cc))
        run(op, [entry([z, y, None, np.array([1.0, 1.0], F32)], [out], n=n, C=Cc, eps=0.0)])
        fig = max(fig, libm_figure_ce(op, z, y, out))
    name = "ce_terms" if op == CE_TERMS else "ce_grad"
    print(f"[head {name} C {Cc}] max err / bound {worst:.3f}; math-library figure {fig:.2f} (budget {R.CE_LSE_U if op == CE_TERMS else R.CE_P_U})")


# ---- GELU + dropout ----------------------------------------------------------------------------------------------------
GELU_N = [1, 255, 256, 257, 5000]
GELU_THR = [0, int(0.1 * 2 ** 24), 2 ** 24 - 1]


gelu_case = R.gelu_case


def check_gelu(op, z, d, key, thr, scale, io, tag):
    n = z.size
    assert (io[n:] == CANARY).all(), ("canary", tag)
    ref, bound, keep = R.gelu_dropout_fwd_ref(z, key, thr, scale) if op == GELU_FWD else R.gelu_dropout_bwd_ref(z, d, key, thr, scale)
    got = io[:n]
    # a dropped element is an exact zero; a kept one is within the bound of gelu(z) scale != 0 (erff(z / sqrt 2) is exactly -1 in
    # fp32 below z ~ -5.4, where the kept value is a zero as well: the bound there is wider than the value)
    assert (got[~keep] == 0).all(), ("keep mask: mix64(key + i) >> 40 >= thr", tag)
    r = R.ratio(got[keep], ref[keep], bound[keep])
    if op == GELU_FWD:
        unit = R.U32 * (np.abs(z.astype(np.float64)) + np.abs(R.gelu64(z))) * float(scale)
    else:
        unit = R.U32 * np.abs(d.astype(np.float64)) * float(scale) * (1.0 + np.abs(R.gelu_grad64(z)))
    # the figure GELU_LIB_U / GELU_GRAD_U were set from: the error beyond the itemised product roundings (u32 |ref| resp. 2 u32 |ref|)
    own = (1 if op == GELU_FWD else 2) * R.U32 * np.abs(ref)
    fig = float((np.maximum(np.abs(got.astype(np.float64) - ref) - own, 0.0)[keep] / unit[keep]).max()) if keep.any() else 0.0
    return r, fig


@pytest.mark.parametrize("op", [GELU_FWD, GELU_BWD], ids=["fwd", "bwd"])
def test_gelu_dropout(op):
    worst, fig = 0.0, 0.0
    for n in GELU_N:
        for thr in GELU_THR:
            for which in (0, 1):
                z, d, key, scale = gelu_case(n, thr, which)
                io = image(n)
                if op == GELU_BWD:
                    io[:n] = d
                run(op, [entry([z], [io], n=n, key=key, thr=thr, scale=scale)])
                r, f = check_gelu(op, z, d, key, thr, scale, io, (n, thr, which))
                worst, fig = max(worst, r), max(fig, f)
                assert r <= 1.0, (n, thr, which, r)
    name = "fwd" if op == GELU_FWD else "bwd"
    print(f"[head gelu_dropout {name}] max err / bound {worst:.3f}; math-library figure {fig:.2f} "
          f"(budget {R.GELU_LIB_U if op == GELU_FWD else R.GELU_GRAD_U})")


# ---- Adam ---------------------------------------------------------------------------------------------------------------
ADAM_N = [1, 255, 256, 257, 1000]
WD_SPECIAL = 1e-3
LR = 1e-3


def adam_ranges(n):
    return [(0, 0), (0, 1), (255, 257), (n - 1, n)]


def check_adam(ins, n, cfg, outs, tag):
    p, g, m, v = ins
    (rp, rm, rv), (Ep, Em, Ev) = R.adam_ref(p, g, m, v, LR, cfg["wd"], cfg["wd_lo"], cfg["wd_hi"], WD_SPECIAL, cfg["step"])
    worst = 0.0
    for o, ref, bound, name in zip(outs, (rp, rm, rv), (Ep, Em, Ev), "pmv"):
        assert (o[n:] == CANARY).all(), ("canary past n in " + name, tag)
        r = R.ratio(o[:n], ref, bound)
        worst = max(worst, r)
        assert r <= 1.0, (name, tag, r)
    return worst


def adam_outs(ins, n):
    outs = [image(n) for _ in range(3)]
    for o, t in zip(outs, (ins[0], ins[2], ins[3])):
        o[:n] = t
    return outs


@pytest.mark.parametrize("n", ADAM_N)
def test_adam(n):
    worst = 0.0
    ins = R.adam_case(n, n)
    for step in (1, 2, 1000):
        for lo, hi in adam_ranges(n):
            for wd in (0.0, 1e-2):
                cfg = dict(wd=wd, wd_lo=lo, wd_hi=hi, step=step)
                outs = adam_outs(ins, n)
                run(ADAM, [entry([ins[1]], outs, n=n, lr=LR, wd_special=WD_SPECIAL, **cfg)])
                worst = max(worst, check_adam(ins, n, cfg, outs, (n, step, lo, hi, wd)))
    print(f"[head adam n {n}] p, m, v max err / bound {worst:.3f}")


# ---- every `_multi` form ---------------------------------------------------------------------------------------------------
def multi_sizes(k, base):
    """k unequal sizes: one empty entry, the largest not first."""
    s = [base[(2 * j + 1) % len(base)] for j in range(k)]
    if k >= 3:
        s[1] = 0
        s[k - 1] = max(base)
        s[0] = min(x for x in base if x > 1)
    return s


def both_ways(op, entries_of):
    """Run the `_multi` launcher on all entries and the single-trial launcher on each; returns the two lists of output lists."""
    multi = entries_of()
    run(op, multi, multi=1)
    solo = entries_of()
    for e in solo:
        if e[0]["n"] > 0 and e[0].get("cols", 1) > 0:
            run(op, [e])
    for j, (em, es) in enumerate(zip(multi, solo)):
        for i, (a, b) in enumerate(zip(em[2], es[2])):
            assert same_bits(a, b), (f"entry {j} out[{i}]: the trial-batched launcher differs from the single-trial one", op)
    return [e[2] for e in multi]


@pytest.mark.parametrize("k", [1, 3, 8])
def test_multi_forms(k):
    worst = {}
    # gelu_dropout forward / backward
    sizes = multi_sizes(k, GELU_N)
    for op in (GELU_FWD, GELU_BWD):
        cases = [gelu_case(max(n, 1), GELU_THR[j % 3], j % 2) for j, n in enumerate(sizes)]

        def mk():
            es = []
            for n, (z, d, key, scale) in zip(sizes, cases):
                io = image(n)
                if op == GELU_BWD:
                    io[:n] = d[:n]
                es.append(entry([z[:n]], [io], n=n, key=key, thr=GELU_THR[len(es) % 3], scale=scale))
            return es
        outs = both_ways(op, mk)
        for j, (n, (z, d, key, scale)) in enumerate(zip(sizes, cases)):
            if n:
                r, _ = check_gelu(op, z[:n], d[:n], key, GELU_THR[j % 3], scale, outs[j][0], (k, j, n))
                assert r <= 1.0, (op, k, j, n, r)
                worst["gelu_dropout"] = max(worst.get("gelu_dropout", 0.0), r)
            else:
                assert (outs[j][0] == CANARY).all()
    # cross entropy
    sizes = multi_sizes(k, CE_N)
    for op in (CE_TERMS, CE_GRAD):
        cfg = [(CE_C[j % 4], j % 2 == 1, 0.1 * (j % 2)) for j in range(k)]
        cases = [R.ce_case(max(n, 1), Cc, 31 * j + n, cw) for j, (n, (Cc, cw, _)) in enumerate(zip(sizes, cfg))]

        def mk():
            es = []
            for n, (Cc, _, eps), (z, y, cw) in zip(sizes, cfg, cases):
                sums = ce_sums(z[:max(n, 1)], y[:max(n, 1)], cw, eps)
                es.append(entry([z[:n], y[:n], cw, sums], [image(n * (2 if op == CE_TERMS else Cc))], n=n, C=Cc, eps=eps))
            return es
        outs = both_ways(op, mk)
        for j, (n, (Cc, _, eps), (z, y, cw)) in enumerate(zip(sizes, cfg, cases)):
            if n:
                r = check_ce(op, z[:n], y[:n], cw, eps, ce_sums(z[:n], y[:n], cw, eps), outs[j][0], (k, j, n))
                assert r <= 1.0, (op, k, j, r)
                worst["ce"] = max(worst.get("ce", 0.0), r)
            else:
                assert (outs[j][0] == CANARY).all()
    # cov_offdiag
    sizes = multi_sizes(k, [32, 64, 96, 100, 256])
    cases = [cov_case(max(n, 1), 50 + j) for j, n in enumerate(sizes)]

    def mk_cov():
        return [entry([c if n else None], [image(n * n), image(n)], n=n, cscale=cs, gscale=gs) for n, (c, cs, gs) in zip(sizes, cases)]
    outs = both_ways(COV_OFFDIAG, mk_cov)
    for j, (n, (c, cs, gs)) in enumerate(zip(sizes, cases)):
        if n:
            r = check_cov(c, n, cs, gs, outs[j][0], outs[j][1], (k, j, n))
            assert r <= 1.0, (k, j, r)
            worst["cov_offdiag"] = max(worst.get("cov_offdiag", 0.0), r)
        else:
            assert (outs[j][0] == CANARY).all() and (outs[j][1] == CANARY).all()
    # colsum (scale 1): an empty entry has cols = 0
    rows_l = multi_sizes(k, [37, 63, 64, 65, 1000])
    cols_l = [[63, 200, 1, 65, 64][j % 5] if rows_l[j] else 0 for j in range(k)]
    cases = [colsum_case(max(r, 1), max(c, 1), 90 + j) for j, (r, c) in enumerate(zip(rows_l, cols_l))]

    def mk_cs():
        return [entry([src if c else None], [image(64 * c), image(c)], n=r, cols=c, ld=ld if c else 0, scale=1.0)
                for r, c, (src, ld) in zip(rows_l, cols_l, cases)]
    outs = both_ways(COLSUM, mk_cs)
    for j, (r_, c, (src, ld)) in enumerate(zip(rows_l, cols_l, cases)):
        if c:
            r = check_colsum(src, r_, c, 1.0, outs[j][0], outs[j][1], (k, j, r_, c))
            assert r <= 1.0, (k, j, r)
            worst["colsum"] = max(worst.get("colsum", 0.0), r)
        else:
            assert (outs[j][0] == CANARY).all() and (outs[j][1] == CANARY).all()
    # add_vec / copy
    sizes = multi_sizes(k, SIZES)
    cases = vec_entries(sizes, 5)

    def mk_vec():
        return [entry([a, b], [image(n)], n=n) for n, (a, b) in zip(sizes, cases)]
    outs = both_ways(ADD_VEC, mk_vec)
    for j, (n, (a, b)) in enumerate(zip(sizes, cases)):
        assert (outs[j][0][n:] == CANARY).all() and same_bits(outs[j][0][:n], a + b if b is not None else a), (k, j)
    # adam
    sizes = multi_sizes(k, ADAM_N)
    cases = [R.adam_case(max(n, 1), 70 + j) for j, n in enumerate(sizes)]
    cfgs = [dict(wd=[0.0, 1e-2][j % 2], step=[1, 2, 1000][j % 3], wd_lo=adam_ranges(max(n, 1))[j % 4][0], wd_hi=adam_ranges(max(n, 1))[j % 4][1])
            for j, n in enumerate(sizes)]

    def mk_adam():
        return [entry([ins[1][:n]], adam_outs([t[:n] for t in ins], n), n=n, lr=LR, wd_special=WD_SPECIAL, **cfg)
                for n, ins, cfg in zip(sizes, cases, cfgs)]
    outs = both_ways(ADAM, mk_adam)
    for j, (n, ins, cfg) in enumerate(zip(sizes, cases, cfgs)):
        if n:
            worst["adam"] = max(worst.get("adam", 0.0), check_adam([t[:n] for t in ins], n, cfg, outs[j], (k, j, n)))
        else:
            assert all((o == CANARY).all() for o in outs[j])
    print(f"[head multi k {k}] every entry = the single-trial launcher bit for bit; max err / bound " +
          ", ".join(f"{n} {v:.3f}" for n, v in worst.items()))


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_harness_refuses_what_a_launcher_would_mishandle():
    lib = _lib.load()
    A, W, b = R.head_gemm_case(8, 8, 64, 1)
    out = np.full((8, 8), CANARY, F32)
    ok = dict(M=8, N=8, N_alloc=8, K=64, lda=64, ldw=0, ldo=8, gelu=0)

    def gemm(entries=None, **kw):
        return head_call(GEMM, entries or [entry([A, W, b], [out])], **{**ok, **kw})
    assert gemm() == 0
    part = image(2 * 64)
    for bad in (dict(M=0), dict(N=0), dict(N=6, N_alloc=6, ldo=8), dict(K=48), dict(K=0), dict(N_alloc=4), dict(lda=66), dict(ldo=10),
                dict(ldw=66), dict(lda=32), dict(ldw=32), dict(ldo=4), dict(gelu=2),
                dict(K=32, splits=2, split_stride=64),                                         # a bias with split-K
                dict(M=9), dict(N=12, N_alloc=12, ldo=12), dict(N_alloc=12)):                  # images smaller than the launch reads / writes
        assert gemm(**bad) == EINVAL, bad
    nb = [entry([A, W, None], [out, part])]
    sk = dict(K=32, ldw=64, splits=2, split_stride=64)
    assert gemm(nb, **sk) == 0
    for bad in (dict(gelu=1), dict(split_stride=66), dict(split_stride=32), dict(ldo=12), dict(K=64), dict(ldw=0), dict(ldw=32)):
        assert gemm(nb, **{**sk, **bad}) == EINVAL, bad
    assert gemm([entry([A, W, None], [out, part[:100]])], **sk) == EINVAL                          # partial image too small
    # struct sizes, op, k
    a = HeadArgs()
    a.struct_bytes = C.sizeof(HeadArgs) - 8
    assert lib.cbas_debug_head_run(C.byref(a)) == EINVAL and lib.cbas_debug_head_run(None) == EINVAL
    x = np.ones(8, F32)
    o = image(8)
    assert head_call(ADD_VEC, [entry([x, x], [o], n=8)]) == 0
    assert head_call(11, [entry([x, x], [o], n=8)]) == EINVAL and head_call(-1, [entry([x, x], [o], n=8)]) == EINVAL
    for k in (0, -1, R.TRAIN_MULTI_MAX + 1):
        assert head_call(ADD_VEC, [entry([x, x], [image(8)], n=8)] * max(k, 1), multi=1, k=k) == EINVAL, k
    for op in (GEMM, TRANSPOSE_PAD, SUB_COLMEAN):
        assert head_call(op, [entry([x, x], [o], n=8, cols=1, ld=1, rows_pad=8)], multi=1, **(ok if op == GEMM else {})) == EINVAL
    # sizes, images
    assert head_call(ADD_VEC, [entry([x, x], [o], n=0)]) == EINVAL and head_call(ADD_VEC, [entry([x, x], [o], n=-1)], multi=1) == EINVAL
    assert head_call(ADD_VEC, [entry([x, x], [o], n=14)]) == EINVAL                             # a and b too small
    assert head_call(ADD_VEC, [entry([x, x], [o[:4]], n=8)]) == EINVAL                          # out too small
    assert head_call(ADD_VEC, [entry([None, x], [o], n=8)]) == EINVAL                           # a missing
    # transpose_pad
    src = np.ones((4, 8), F32)
    tp = dict(n=4, cols=8, ld=8, rows_pad=4)
    assert head_call(TRANSPOSE_PAD, [entry([src], [image(32)], **tp)]) == 0
    for bad in (dict(rows_pad=3), dict(ld=7), dict(cols=0), dict(n=0), dict(n=5), dict(rows_pad=16)):
        assert head_call(TRANSPOSE_PAD, [entry([src], [image(32)], **{**tp, **bad})]) == EINVAL, bad
    # cross entropy: C, labels
    z, y, cw = R.ce_case(5, 9, 1, True)
    sums = np.ones(2, F32)
    for op, osz in ((CE_TERMS, 10), (CE_GRAD, 45)):
        assert head_call(op, [entry([z, y, cw, sums], [image(osz)], n=5, C=9, eps=0.1)]) == 0
        for lab in (-1, 9, 64):
            yb = y.copy()
            yb[3] = lab
            assert head_call(op, [entry([z, yb, cw, sums], [image(osz)], n=5, C=9, eps=0.1)]) == EINVAL, lab
            assert head_call(op, [entry([z, y, cw, sums], [image(osz)], n=5, C=9, eps=0.1), entry([z, yb, cw, sums], [image(osz)], n=5, C=9)],
                             multi=1) == EINVAL
        big = np.zeros((2, 65), F32)
        assert head_call(op, [entry([big, y[:2] * 0, None, sums], [image(130)], n=2, C=65)]) == EINVAL
        assert head_call(op, [entry([z, y, cw, sums], [image(osz)], n=5, C=0)]) == EINVAL
        assert head_call(op, [entry([z, y, cw[:4], sums], [image(osz)], n=5, C=9)]) == EINVAL       # cw shorter than C
    assert head_call(CE_GRAD, [entry([z, y, cw, None], [image(45)], n=5, C=9)]) == EINVAL            # sums missing
    # colsum, cov, gelu, adam
    s2 = np.ones((4, 8), F32)
    assert head_call(COLSUM, [entry([s2], [image(64 * 8), image(8)], n=4, cols=8, ld=8, scale=0.5)]) == 0
    assert head_call(COLSUM, [entry([s2], [image(64 * 8), image(8)], n=4, cols=8, ld=8, scale=0.5)], multi=1) == EINVAL
    assert head_call(COLSUM, [entry([s2], [image(64 * 8), image(8)], n=4, cols=8, ld=6, scale=1.0)]) == EINVAL
    assert head_call(COLSUM, [entry([s2], [image(63 * 8), image(8)], n=4, cols=8, ld=8, scale=1.0)], out_bytes={(0, 0): 63 * 8 * 4}) == EINVAL
    assert head_call(COLSUM, [entry([s2], [image(64 * 8), image(8)], n=5, cols=8, ld=8, scale=1.0)]) == EINVAL
    assert head_call(COV_OFFDIAG, [entry([np.ones((4, 4), F32)], [image(16), image(3)], n=4)], out_bytes={(0, 1): 12}) == EINVAL
    zz = np.ones(8, F32)
    assert head_call(GELU_FWD, [entry([zz], [image(8)], n=9, scale=1.0)]) == EINVAL
    assert head_call(GELU_BWD, [entry([zz], [image(8)], n=8, scale=1.0, thr=2 ** 24 + 1)]) == EINVAL
    ins = R.adam_case(8, 1)
    ad = dict(n=8, lr=LR, wd=0.0, wd_lo=0, wd_hi=1, wd_special=WD_SPECIAL, step=1)
    assert head_call(ADAM, [entry([ins[1]], adam_outs(ins, 8), **ad)]) == 0
    assert head_call(ADAM, [entry([ins[1]], adam_outs(ins, 8), **{**ad, "step": 0})]) == EINVAL
    assert head_call(ADAM, [entry([ins[1]], adam_outs(ins, 8), **{**ad, "n": 16})]) == EINVAL
    assert head_call(ADAM, [entry([ins[1]], adam_outs(ins, 8)[:2], **ad)]) == EINVAL                # v missing
    assert head_call(ADAM, [entry([ins[1]], adam_outs(ins, 8), **ad), entry([ins[1]], adam_outs(ins, 8), **{**ad, "wd_special": 0.5})],
                     multi=1) == EINVAL
