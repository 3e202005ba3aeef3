"""fp64 restatements of what csrc/wide_gemm.hip computes, with an a-priori rounding bound per element, and the guard-band harness
the direct kernel tests (tests/test_wide_kernels.py) carve their device operands from.

Written from the contract in include/careless_hip.h (the block starting at "Activation buffers are row-major") and the reference's
MetadataScaler.call / NormalLayer / ImageLayer: h_l = LeakyReLU(h_{l-1} W_l + b_l), (loc, raw) = h_L Wo + bo, sigma = bijector(raw) + eps.
Nothing here calls oracle/elbo_oracle.py; every function takes the fp32 arrays the device gets and converts them to fp64.

The bound.  A dot product of length m accumulated in fp32 in ANY order, with or without fused multiply-adds, differs from the exact one
by at most gamma(m) * sum |a_i| |b_i|, gamma(m) = m u / (1 - m u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms,
section 3.1).  m = the contraction length + 4: the bias, the activation's multiply, the partial sum cl_reduce_partials adds, the store.
DESIGN 4.1: v_mfma_f32_16x16x4_f32 is bit-equal to an fmaf chain, so the bound is derived, not measured.  Chains (two layers, a head
behind a layer, a mask recomputed from the first layer) carry the error of their input to first order: e_out = gamma |a| |b| + e_in |b|.
(sigma, d sigma / d raw) behind the bijector get 1e-5 relative on top, the figure tests/test_host_math.py holds cl_scale_bij to.
"""
from __future__ import annotations

import numpy as np

from tests.ref_step import f64

U = 2.0 ** -24
BIJ_EXP, BIJ_SOFTPLUS = 0, 1
BIJ_RTOL = 1e-5


def gamma(m):
    return m * U / (1.0 - m * U)


def slope(h, leak):
    """LeakyReLU'(h) as every kernel takes it: 1 where h > 0, the leak elsewhere (at +0.0 and -0.0 too)"""
    return np.where(f64(h) > 0.0, 1.0, float(leak))


def lrelu(z, leak):
    return np.where(z > 0.0, z, float(leak) * z)


def _dot(A, B, eA=None):
    """A @ B in fp64, the rounding bound of its fp32 evaluation, propagated error of A (first order)"""
    A, B = f64(A), f64(B)
    v = A @ B
    s = np.abs(A) @ np.abs(B)
    e = np.zeros_like(v) if eA is None else f64(eA) @ np.abs(B)
    return v, s, e


# ---- forward ---------------------------------------------------------------------------------------------------------------------
def dense_forward(X, Wt, b, leak, act=1, eX=None):
    """Y = act(X Wt^T + b); returns (Y, bound, Z) -- Z the pre-activations"""
    z, s, e = _dot(X, f64(Wt).T, eX)
    z = z + f64(b)
    bound = gamma(f64(X).shape[1] + 4) * (s + np.abs(f64(b))) + e
    y = lrelu(z, leak) if act else z
    return y, bound, z            # (LeakyReLU is 1-Lipschitz: the bound of Z holds for Y; its multiply is one of the + 4)


def bijector(raw, kind):
    """(bijector(raw), its derivative, |second derivative|) of the Dense(2) head's scale bijectors (exp, softplus)"""
    raw = f64(raw)
    if kind == BIJ_EXP:
        ex = np.exp(raw)
        return ex, ex, ex
    sg = 1.0 / (1.0 + np.exp(-raw))
    return np.logaddexp(0.0, raw), sg, sg * (1.0 - sg)


def head_forward(H, head, kind, eps, eH=None):
    """head = [Wo^T (2 x w) | bo (2)]; returns dict of (value, bound) for loc, sig, dsd (= d sigma / d raw)"""
    H = f64(H)
    w = H.shape[1]
    head = f64(head)
    Wo, bo = head[:2 * w].reshape(2, w), head[2 * w:2 * w + 2]
    raw, s, e = _dot(H, Wo.T, eH)
    raw = raw + bo
    braw = gamma(w + 4) * (s + np.abs(bo)) + e
    sg, d1, d2 = bijector(raw[:, 1], kind)
    sigma = sg + eps
    return {"loc": (raw[:, 0], braw[:, 0]),
            "sig": (sigma, d1 * braw[:, 1] + BIJ_RTOL * np.abs(sigma)),
            "dsd": (d1, d2 * braw[:, 1] + BIJ_RTOL * np.abs(d1)),
            "raw": (raw, braw)}


def dense_forward_head(X, Wt, b, leak, head, kind, eps):
    y, by, _ = dense_forward(X, Wt, b, leak, 1)
    out = head_forward(y, head, kind, eps, eH=by)
    out["Y"] = (y, by)
    return out


def first_layer(X0, Wt0, b0, leak):
    """the recomputed first layer: (h_0, bound, pre-activations z_0)"""
    return dense_forward(X0, Wt0, b0, leak, 1)


def near_zero(X0, Wt0, b0):
    """number of first-layer pre-activations that lie inside their own rounding bound (either branch of the mask is legitimate there)"""
    _, bound, z = dense_forward(X0, Wt0, b0, 0.0, 1)
    return int(np.count_nonzero(np.abs(z) <= bound))


def dense2_forward(X0, Wt0, b0, Wt1, b1, leak, head=None, kind=0, eps=0.0):
    h0, e0, _ = first_layer(X0, Wt0, b0, leak)
    y, by, _ = dense_forward(h0, Wt1, b1, leak, 1, eX=e0)
    out = {"Y": (y, by)}
    if head is not None:
        out.update(head_forward(y, head, kind, eps, eH=by))
    return out


# ---- backward --------------------------------------------------------------------------------------------------------------------
def dense_dgrad(dZ, Wt, Hprev, leak, edZ=None):
    """dX = (dZ Wt) * LeakyReLU'(Hprev)   (Hprev None: no mask)"""
    v, s, e = _dot(dZ, Wt, edZ)
    m = 1.0 if Hprev is None else slope(Hprev, leak)
    return v * m, (gamma(f64(dZ).shape[1] + 4) * s + e) * m


def dense_wgrad(dZ, H, edZ=None, eH=None):
    """flat [dWt (out x in) | db (out)] = [dZ^T H | column sums of dZ]"""
    dZ, H = f64(dZ), f64(H)
    n = dZ.shape[0]
    g = gamma(n + 4)
    dW = dZ.T @ H
    bW = g * (np.abs(dZ).T @ np.abs(H))
    db = dZ.sum(0)
    bb = g * np.abs(dZ).sum(0)
    if edZ is not None:
        bW = bW + f64(edZ).T @ np.abs(H)
        bb = bb + f64(edZ).sum(0)
    if eH is not None:
        bW = bW + np.abs(dZ).T @ f64(eH)
    return np.concatenate([dW.ravel(), db]), np.concatenate([bW.ravel(), bb])


def head_dz(H, head, g0, g1, leak, eg1=None):
    """dZ_L = (g0 Wo[0] + g1 Wo[1]) * LeakyReLU'(h_L): a length-2 contraction per element"""
    H = f64(H)
    w = H.shape[1]
    Wo = f64(head)[:2 * w].reshape(2, w)
    g0, g1 = f64(g0)[:, None], f64(g1)[:, None]
    m = slope(H, leak)
    dz = (g0 * Wo[0] + g1 * Wo[1]) * m
    b = gamma(2 + 4) * (np.abs(g0) * np.abs(Wo[0]) + np.abs(g1) * np.abs(Wo[1]))
    if eg1 is not None:
        b = b + f64(eg1)[:, None] * np.abs(Wo[1])
    return dz, b * m


def head_grads(H, g0, g1, eg1=None):
    """flat [dWo (2 x w) | dbo (2)] = [g0^T H, g1^T H | sum g0, sum g1]"""
    H, g0, g1 = f64(H), f64(g0), f64(g1)
    n = H.shape[0]
    g = gamma(n + 4)
    e1 = np.zeros_like(g1) if eg1 is None else f64(eg1)
    aH = np.abs(H)
    v = np.concatenate([g0 @ H, g1 @ H, [g0.sum(), g1.sum()]])
    b = np.concatenate([g * (np.abs(g0) @ aH), g * (np.abs(g1) @ aH) + e1 @ aH, [g * np.abs(g0).sum(), g * np.abs(g1).sum() + e1.sum()]])
    return v, b


def head_backward(H, head, dO, kind, eps, leak):
    """cl_wide_head_backward: the head recomputes raw sigma from h_L; returns dict of (value, bound) for dZ and the flat head gradient"""
    hf = head_forward(H, head, kind, eps)
    dsd, edsd = hf["dsd"]
    dO = f64(dO)
    g0, g1 = dO[:, 0], dO[:, 1] * dsd
    eg1 = np.abs(dO[:, 1]) * edsd + U * np.abs(g1)
    return {"dZ": head_dz(H, head, g0, g1, leak, eg1), "dhead": head_grads(H, g0, g1, eg1)}


def fused_head_g(dO, dsd):
    """g of the fused head backward (dsig_draw an input): g1 = dO[:, 1] * dsd is one rounded product"""
    dO = f64(dO)
    g1 = dO[:, 1] * f64(dsd)
    return dO[:, 0], g1, U * np.abs(g1)


def dense_wgrad_head(Htop, head, dO, dsd, leak, H):
    g0, g1, eg1 = fused_head_g(dO, dsd)
    dz, edz = head_dz(Htop, head, g0, g1, leak, eg1)
    return {"partials": dense_wgrad(dz, H, edZ=edz), "dhead": head_grads(Htop, g0, g1, eg1)}


def dense_dgrad_head(Htop, head, dO, dsd, Wt, Hprev, leak):
    g0, g1, eg1 = fused_head_g(dO, dsd)
    dz, edz = head_dz(Htop, head, g0, g1, leak, eg1)
    return dense_dgrad(dz, Wt, Hprev, leak, edZ=edz)


def dense_dgrad_pre(dZ, Wt, X0, Wt0, b0, leak):
    """layer 1's dgrad behind the mask of the recomputed first layer (the sign of h_0 is the sign of its pre-activation)"""
    _, _, z0 = first_layer(X0, Wt0, b0, leak)
    return dense_dgrad(dZ, Wt, z0, leak)


def dense_wgrad_pre(dZ, X0, Wt0, b0, leak):
    h0, e0, _ = first_layer(X0, Wt0, b0, leak)
    return dense_wgrad(dZ, h0, eH=e0)


def dense_dgrad_pre_wgrad0(dZ, Wt, X0, Wt0, b0, leak):
    """the first layer's flat weight gradient [dWt_0 (w x d0) | db_0 (w)] from dZ_0 = dgrad_pre, which is never stored"""
    dz0, e0 = dense_dgrad_pre(dZ, Wt, X0, Wt0, b0, leak)
    return dense_wgrad(dz0, X0, edZ=e0)


# ---- grouped (per-image) layers: W[g] (out, in), b[g]; rows seg[g] .. seg[g+1] -----------------------------------------------------
def image_forward(X, W, b, seg, leak):
    X = f64(X)
    y, bd = np.zeros((X.shape[0], f64(W).shape[1])), np.zeros((X.shape[0], f64(W).shape[1]))
    for g in range(len(seg) - 1):
        r = slice(int(seg[g]), int(seg[g + 1]))
        if r.stop > r.start:
            y[r], bd[r], _ = dense_forward(X[r], W[g], b[g], leak, 1)
    return y, bd


def image_dgrad(dZ, W, seg, Hprev, leak):
    dZ = f64(dZ)
    v, bd = np.zeros((dZ.shape[0], f64(W).shape[2])), np.zeros((dZ.shape[0], f64(W).shape[2]))
    for g in range(len(seg) - 1):
        r = slice(int(seg[g]), int(seg[g + 1]))
        if r.stop > r.start:
            v[r], bd[r] = dense_dgrad(dZ[r], W[g], None if Hprev is None else Hprev[r], leak)
    return v, bd


def image_wgrad(dZ, H, seg):
    """(dW [G][out][in], db [G][out]) and their bounds; an empty group's gradients are zero"""
    dZ, H = f64(dZ), f64(H)
    G, w = len(seg) - 1, dZ.shape[1]
    dW, bW, db, bb = np.zeros((G, w, w)), np.zeros((G, w, w)), np.zeros((G, w)), np.zeros((G, w))
    for g in range(G):
        r = slice(int(seg[g]), int(seg[g + 1]))
        if r.stop > r.start:
            v, e = dense_wgrad(dZ[r], H[r])
            dW[g], bW[g], db[g], bb[g] = v[:w * w].reshape(w, w), e[:w * w].reshape(w, w), v[w * w:], e[w * w:]
    return (dW, bW), (db, bb)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def normals(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def layer(rng, n_out, n_in):
    """(Wt [out][in] scaled by 1 / sqrt(fan_in), b [out]) as fp32"""
    return (normals(rng, n_out, n_in) / np.float32(np.sqrt(n_in))).astype(np.float32), normals(rng, n_out)


def head_params(rng, w):
    return np.concatenate([(normals(rng, 2, w) / np.float32(np.sqrt(w))).ravel(), 0.3 * normals(rng, 2)]).astype(np.float32)


def with_zeros(rng, H, k=6):
    """a stored mask with a handful of exact +0.0 and -0.0 entries (the derivative there is the leak)"""
    H = np.array(H, dtype=np.float32)
    flat = H.reshape(-1)
    idx = rng.choice(flat.size, size=min(k, flat.size), replace=False)
    flat[idx[::2]] = np.float32(0.0)
    flat[idx[1::2]] = np.float32(-0.0)
    return H


def pre_problem(seed, n, d0, w):
    rng = np.random.default_rng(seed)
    X0 = normals(rng, n, d0)
    Wt0, b0 = layer(rng, w, d0)
    return X0, Wt0, b0, rng


def pre_seed(base, n, d0, w, tries=200):
    """the first seed >= base whose first-layer pre-activations all lie outside their own rounding bound -- found from the reference alone"""
    for s in range(base, base + tries):
        X0, Wt0, b0, _ = pre_problem(s, n, d0, w)
        if near_zero(X0, Wt0, b0) == 0:
            return s
    raise AssertionError(f"no seed in [{base}, {base + tries}) without a first-layer pre-activation inside its rounding bound (n={n}, d0={d0}, w={w})")


# Seeds found by a longer search than `pre_seed` makes at collection (same criterion, the reference alone; n = n_long at the MI355X's
# 256 CUs): a seed without a pre-activation inside its bound is about one in a few hundred there.
_SEEDS = {(65925, 8, 120): 813546}


def pre_case_seed(n, d0, w):
    """the seed of the recomputed-first-layer case (n rows, d0 metadata columns, first-layer width w)"""
    key = (int(n), int(d0), int(w))
    if key not in _SEEDS:
        _SEEDS[key] = pre_seed(100000 * d0 + 100 * w + n % 97, n, d0, w)
    return _SEEDS[key]


N_ROWS = (1, 129, 677)
N_ROWS_WGRAD = (40, 677, 5000)
D0S = (1, 8, 15)
LONG_D0S = (1, 8)   # the long cases of the recomputed-mask forms have 8 M pre-activations: the expected number inside their own bound per seed is
                    # about 2 at d0 = 1 and 5 at d0 = 8 (a clean seed exists and is recorded in _SEEDS), about 19 at d0 = 15 -- one clean seed in
                    # e^19: out of reach under "no element excluded", so d0 = 15 runs at n <= 677 only


def n_long(cus):
    """rows at which some waves of the streaming kernels walk two 16-row blocks, some one, and the last block is ragged"""
    return 128 * (2 * cus) + 128 * 3 + 5


# (n, d0, n_out, n_in) of every case whose mask comes from the recomputed first layer (width n_in), as checked on the CPU: the long
# case at the MI355X's 256 CUs
PRE_DGRAD_LAYERS = ((100, 100), (120, 120), (80, 65), (70, 96))          # (n_out, n_in): in -> out = 100 -> 100, 120 -> 120, 65 -> 80, 96 -> 70
PRE_WGRAD_LAYERS = ((100, 100), (120, 120), (65, 80))                     # (n_out, n_in)
PRE_CASES_CPU = ([(n, d0, no, ni) for (no, ni) in PRE_DGRAD_LAYERS for d0 in D0S for n in N_ROWS] + [(n_long(256), d0, 120, 120) for d0 in LONG_D0S] +
                 [(n, d0, no, ni) for (no, ni) in PRE_WGRAD_LAYERS for d0 in D0S for n in N_ROWS_WGRAD])


# ---- harness ---------------------------------------------------------------------------------------------------------------------
GUARD_ROWS = 32
SENTINEL = np.float32(-7.25e30)


class Arena:
    """Every device operand of a call carved out of ONE allocation, 32 guard rows of a finite sentinel in front of and behind each.

    Inputs: data columns as given, padding columns [width, ld) zero (the contract).  Outputs: data columns pre-filled with the
    sentinel, padding columns zero.  Partial buffers: all sentinel.  `verify` then asserts, bit for bit, that nothing outside the
    outputs' data columns changed (guards, inputs, padding columns of inputs), that every output data element was written, that
    every output padding column is exactly 0.0, and that the named slots of the partial buffers were written."""

    def __init__(self, device):
        self.device = device
        self.ops = {}
        self.size = 0
        self.base = None

    def _add(self, name, kind, rows, width, ld, misalign, data):
        ld = width if ld is None else ld
        assert ld >= width and name not in self.ops
        guard = GUARD_ROWS * max(ld, 1)
        start = (self.size + guard + 3) // 4 * 4 + misalign            # data 16-byte aligned, or `misalign` floats off it
        self.ops[name] = dict(kind=kind, rows=rows, width=width, ld=ld, start=start, data=data)
        self.size = start + rows * ld + guard
        return self

    def input(self, name, a, ld=None, misalign=0):
        a = np.asarray(a)
        if a.dtype != np.float32:
            a = np.ascontiguousarray(a, dtype=np.int32).view(np.float32)      # int operands (seg, tiles, the stop flag): the same bits
        a = a.reshape(1, -1) if a.ndim == 1 else a.reshape(a.shape[0], -1)
        return self._add(name, "in", a.shape[0], a.shape[1], ld, misalign, a)

    def output(self, name, rows, width, ld=None, misalign=0):
        return self._add(name, "out", rows, width, ld, misalign, None)

    def partial(self, name, nfloats):
        return self._add(name, "part", 1, nfloats, None, 0, None)

    def accum(self, name, nfloats):
        """zeros that a call adds to (cl_reduce_partials' grad_mlp)"""
        return self._add(name, "acc", 1, nfloats, None, 0, None)

    def build(self):
        import torch
        img = np.full(self.size + 4, SENTINEL, dtype=np.float32)
        own = np.zeros(self.size + 4, dtype=bool)                      # elements a call may (and must) write
        for o in self.ops.values():
            v = img[o["start"]:o["start"] + o["rows"] * o["ld"]].reshape(o["rows"], o["ld"])
            m = own[o["start"]:o["start"] + o["rows"] * o["ld"]].reshape(o["rows"], o["ld"])
            if o["kind"] == "in":
                v[:, :o["width"]] = o["data"]
                v[:, o["width"]:] = 0.0
            elif o["kind"] == "out":
                v[:, o["width"]:] = 0.0
                m[:] = True                                            # (the padding columns have their own test: zero of either sign)
            else:
                m[:] = True
                if o["kind"] == "acc":
                    v[:] = 0.0
        self.img, self.own = img, own
        self.base = torch.from_numpy(img.copy()).to(self.device)
        return self

    def ptr(self, name):
        return None if name is None else self.base.data_ptr() + 4 * self.ops[name]["start"]

    def ld(self, name):
        return self.ops[name]["ld"]

    def download(self):
        self.got = self.base.cpu().numpy()
        return self.got

    def get(self, name):
        o = self.ops[name]
        return self.got[o["start"]:o["start"] + o["rows"] * o["ld"]].reshape(o["rows"], o["ld"])[:, :o["width"]]

    def verify(self, written=None, untouched=False):
        """written: {partial name: number of leading floats that must have been written} (default: all of every partial buffer);
        untouched: the call must have written NOTHING (a raised stop flag)"""
        got = self.download()
        gi, ii = got.view(np.int32), self.img.view(np.int32)
        if untouched:
            bad = np.flatnonzero(gi != ii)
            assert bad.size == 0, f"{bad.size} elements written although nothing may be, first at float {bad[0]} ({self._where(bad[0])})"
            return
        bad = np.flatnonzero((gi != ii) & ~self.own)
        assert bad.size == 0, f"{bad.size} elements outside the outputs changed, first at float {bad[0]} ({self._where(bad[0])}): {got[bad[0]]!r}"
        sent = SENTINEL.view(np.int32)
        for name, o in self.ops.items():
            blk = got[o["start"]:o["start"] + o["rows"] * o["ld"]].reshape(o["rows"], o["ld"])
            if o["kind"] == "out":
                miss = np.argwhere(blk[:, :o["width"]].view(np.int32) == sent)
                assert miss.size == 0, f"{name}: {len(miss)} data elements never written, first (row, column) {tuple(miss[0])}"
                pad = blk[:, o["width"]:]
                assert np.all(pad == 0.0), f"{name}: padding columns [{o['width']}, {o['ld']}) not zero after the call"
            elif o["kind"] == "part":
                k = o["width"] if written is None or name not in written else int(written[name])
                miss = np.flatnonzero(blk[0, :k].view(np.int32) == sent)
                assert miss.size == 0, f"{name}: {miss.size} of {k} partial slots never written, first {miss[0]}"

    def _where(self, at):
        for name, o in self.ops.items():
            g = GUARD_ROWS * max(o["ld"], 1)
            if o["start"] - g <= at < o["start"] + o["rows"] * o["ld"] + g:
                rel = at - o["start"]
                return f"{name}: row {rel // o['ld']}, column {rel % o['ld']}" if 0 <= rel < o["rows"] * o["ld"] else f"guard band of {name}"
        return "between operands"


def assert_within(got, ref, bound, what, entry=None):
    """|got - ref| <= bound element by element (no max-norm scaling); returns the largest error / bound ratio"""
    got, ref, bound = f64(got), f64(ref), f64(bound)
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    assert np.all(np.isfinite(got)), f"{what}: non-finite values"
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0.0, err / bound, 0.0)
    worst = float(ratio.max()) if ratio.size else 0.0
    what = what if entry is None else f"{entry}: {what}"
    bad = np.argwhere(err > bound)
    assert bad.size == 0, (f"{what}: {len(bad)} of {err.size} elements outside their rounding bound, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r}, "
                           f"reference {ref[tuple(bad[0])]!r}, bound {bound[tuple(bad[0])]:.3g}; largest error / bound {worst:.3g}")
    return worst
