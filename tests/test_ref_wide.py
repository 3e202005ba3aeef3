"""The fp64 references of tests/ref_wide.py checked against torch.autograd of their own forward functions (CPU, no device), the
guard-band harness checked against writes it must catch, and the seeds of the recomputed-first-layer cases checked to leave no
pre-activation inside its rounding bound."""
import numpy as np
import pytest
import torch

from tests import ref_wide as R

LEAK = 0.01
SHAPES = [(7, 5, 9), (33, 20, 12), (50, 17, 17)]      # rows, in, out
T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))


def t_lrelu(z):
    return torch.where(z > 0, z, LEAK * z)


def t_bij(raw, kind):
    return torch.exp(raw) if kind == R.BIJ_EXP else torch.nn.functional.softplus(raw)


def close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert np.max(np.abs(a - b)) <= 1e-12 * max(1.0, float(np.max(np.abs(b)))), float(np.max(np.abs(a - b)))


@pytest.mark.parametrize("n,k,m", SHAPES)
def test_dgrad_and_wgrad_equal_autograd(n, k, m):
    rng = np.random.default_rng(n)
    zp, (Wt, b), dZ = R.normals(rng, n, k), R.layer(rng, m, k), R.normals(rng, n, m)
    zt, Wtt, bt = T(zp).requires_grad_(True), T(Wt).requires_grad_(True), T(b).requires_grad_(True)
    h = t_lrelu(zt)
    y = h @ Wtt.T + bt
    close(y.detach().numpy(), R.dense_forward(h.detach().numpy(), Wt, b, LEAK, 0)[0])
    close(t_lrelu(y).detach().numpy(), R.dense_forward(h.detach().numpy(), Wt, b, LEAK, 1)[0])
    gz, gW, gb = torch.autograd.grad((y * T(dZ)).sum(), [zt, Wtt, bt])
    close(R.dense_dgrad(dZ, Wt, h.detach().numpy(), LEAK)[0], gz.numpy())
    close(R.dense_wgrad(dZ, h.detach().numpy())[0], np.concatenate([gW.numpy().ravel(), gb.numpy()]))
    xt = T(zp).requires_grad_(True)                                    # no mask: d / d input of a linear layer
    gx, = torch.autograd.grad(((xt @ Wtt.detach().T + bt.detach()) * T(dZ)).sum(), [xt])
    close(R.dense_dgrad(dZ, Wt, None, LEAK)[0], gx.numpy())


@pytest.mark.parametrize("kind", [R.BIJ_EXP, R.BIJ_SOFTPLUS])
@pytest.mark.parametrize("n,k,m", SHAPES)
def test_head_backward_equals_autograd(n, k, m, kind):
    rng = np.random.default_rng(100 + n)
    z, head, dO, eps = R.normals(rng, n, m), R.head_params(rng, m), R.normals(rng, n, 2), 1e-7
    zt, ht = T(z).requires_grad_(True), T(head).requires_grad_(True)
    h = t_lrelu(zt)
    raw = h @ ht[:2 * m].reshape(2, m).T + ht[2 * m:]
    loc, sig = raw[:, 0], t_bij(raw[:, 1], kind) + eps
    f = R.head_forward(h.detach().numpy(), head, kind, eps)
    close(f["loc"][0], loc.detach().numpy())
    close(f["sig"][0], sig.detach().numpy())
    gz, gh = torch.autograd.grad((loc * T(dO[:, 0]) + sig * T(dO[:, 1])).sum(), [zt, ht])
    bw = R.head_backward(h.detach().numpy(), head, dO, kind, eps, LEAK)
    close(bw["dZ"][0], gz.numpy())
    close(bw["dhead"][0], gh.numpy())
    # the fused forms take d sigma / d raw as an input: the same numbers
    Wt, b = R.layer(rng, m, k)
    Hin = R.normals(rng, n, k)
    close(R.dense_wgrad_head(h.detach().numpy(), head, dO, f["dsd"][0], LEAK, Hin)["partials"][0], R.dense_wgrad(bw["dZ"][0], Hin)[0])
    close(R.dense_wgrad_head(h.detach().numpy(), head, dO, f["dsd"][0], LEAK, Hin)["dhead"][0], gh.numpy())
    close(R.dense_dgrad_head(h.detach().numpy(), head, dO, f["dsd"][0], Wt, Hin, LEAK)[0], R.dense_dgrad(bw["dZ"][0], Wt, Hin, LEAK)[0])


@pytest.mark.parametrize("n,d0,w", [(7, 1, 9), (33, 8, 20), (50, 15, 17)])
def test_recomputed_first_layer_forms_equal_autograd(n, d0, w):
    X0, Wt0, b0, rng = R.pre_problem(R.pre_seed(5, n, d0, w), n, d0, w)
    (Wt1, b1), dZ, head = R.layer(rng, w, w), R.normals(rng, n, w), R.head_params(rng, w)
    W0t, b0t, W1t, b1t = (T(a).requires_grad_(True) for a in (Wt0, b0, Wt1, b1))
    h0 = t_lrelu(T(X0) @ W0t.T + b0t)
    z1 = h0 @ W1t.T + b1t
    out = R.dense2_forward(X0, Wt0, b0, Wt1, b1, LEAK, head, R.BIJ_SOFTPLUS, 1e-7)
    close(out["Y"][0], t_lrelu(z1).detach().numpy())
    close(out["loc"][0], R.head_forward(out["Y"][0], head, R.BIJ_SOFTPLUS, 1e-7)["loc"][0])
    gW0, gb0, gW1, gb1, gh0 = torch.autograd.grad((z1 * T(dZ)).sum(), [W0t, b0t, W1t, b1t, h0])
    close(R.dense_wgrad_pre(dZ, X0, Wt0, b0, LEAK)[0], np.concatenate([gW1.numpy().ravel(), gb1.numpy()]))
    close(R.dense_dgrad_pre_wgrad0(dZ, Wt1, X0, Wt0, b0, LEAK)[0], np.concatenate([gW0.numpy().ravel(), gb0.numpy()]))
    close(R.dense_dgrad_pre(dZ, Wt1, X0, Wt0, b0, LEAK)[0], gh0.numpy() * R.slope(h0.detach().numpy(), LEAK))


@pytest.mark.parametrize("w", [5, 12, 17])
def test_grouped_forms_equal_autograd(w):
    rng = np.random.default_rng(w)
    sizes = [0, 1, 4, 0, 3]
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n, G = int(seg[-1]), len(sizes)
    zp, W, b, dZ = R.normals(rng, n, w), R.normals(rng, G, w, w) / np.float32(np.sqrt(w)), R.normals(rng, G, w), R.normals(rng, n, w)
    zt, Wt_, bt = T(zp).requires_grad_(True), T(W).requires_grad_(True), T(b).requires_grad_(True)
    h = t_lrelu(zt)
    gid = np.repeat(np.arange(G), sizes)
    z = torch.einsum("ni,noi->no", h, Wt_[gid]) + bt[gid]
    close(R.image_forward(h.detach().numpy(), W, b, seg, LEAK)[0], t_lrelu(z).detach().numpy())
    gz, gW, gb = torch.autograd.grad((z * T(dZ)).sum(), [zt, Wt_, bt])
    close(R.image_dgrad(dZ, W, seg, h.detach().numpy(), LEAK)[0], gz.numpy())
    (dW, _), (db, _) = R.image_wgrad(dZ, h.detach().numpy(), seg)
    close(dW, gW.numpy())
    close(db, gb.numpy())
    assert not dW[0].any() and not db[3].any()


def test_bounds_hold_for_an_fp32_evaluation_and_catch_a_dropped_term():
    """The bound is far above what fp32 numpy does and far below one dropped term of the contraction."""
    rng = np.random.default_rng(3)
    X, (Wt, b) = R.normals(rng, 64, 100), R.layer(rng, 112, 100)
    y, bound, _ = R.dense_forward(X, Wt, b, LEAK, 0)
    y32 = X @ Wt.T + b
    assert np.all(np.abs(y32 - y) <= bound)
    Xd = X.copy(); Xd[:, 37] = 0.0
    yd = R.dense_forward(Xd, Wt, b, LEAK, 0)[0]
    assert np.mean(np.abs(yd - y) > bound) > 0.99
    assert R.slope(np.float32(-0.0), LEAK) == LEAK and R.slope(np.float32(0.0), LEAK) == LEAK


def test_masks_with_exact_zeros():
    H = R.with_zeros(np.random.default_rng(0), R.normals(np.random.default_rng(1), 9, 7))
    z = H[H == 0.0]
    assert z.size == 6 and np.signbit(z).sum() == 3


def test_arena_sees_what_it_must():
    a = R.Arena("cpu").input("X", np.ones((3, 5), np.float32), ld=8).output("Y", 3, 5, ld=8).partial("P", 6).input("seg", np.array([0, 3], np.int32)).build()
    assert a.ptr("X") % 16 == 0 and a.ptr("Y") % 16 == 0 and a.ptr(None) is None
    oy, op = a.ops["Y"], a.ops["P"]
    y = a.base[oy["start"]:oy["start"] + 24].view(3, 8)
    with pytest.raises(AssertionError, match="never written"):
        a.verify()
    a.verify(untouched=True)
    y[:, :5] = 2.0
    a.base[op["start"]:op["start"] + 4] = 1.0
    with pytest.raises(AssertionError, match="partial slots never written"):
        a.verify()
    a.verify(written={"P": 4})
    assert np.all(a.get("Y") == 2.0) and a.get("seg").view(np.int32).tolist() == [[0, 3]]
    y[1, 6] = 3.0
    with pytest.raises(AssertionError, match="padding columns"):
        a.verify(written={"P": 4})
    y[1, 6] = 0.0
    a.base[oy["start"] - 1] = 0.0                                    # the last element of the guard band in front of Y
    with pytest.raises(AssertionError, match="guard band of Y"):
        a.verify(written={"P": 4})
    a.base[oy["start"] - 1] = float(R.SENTINEL)
    a.base[a.ops["X"]["start"] + 5] = 1.0                            # a padding column of an input
    with pytest.raises(AssertionError, match="X: row 0, column 5"):
        a.verify(written={"P": 4})
    with pytest.raises(AssertionError, match="written although nothing may be"):
        a.verify(untouched=True)
    m = R.Arena("cpu").input("X", np.ones((2, 5), np.float32), misalign=1).build()
    assert m.ptr("X") % 16 == 4


@pytest.mark.parametrize("n,d0,n_out,n_in", R.PRE_CASES_CPU)
def test_pre_seeds_leave_no_pre_activation_inside_its_bound(n, d0, n_out, n_in):
    s = R.pre_case_seed(n, d0, n_in)
    X0, Wt0, b0, _ = R.pre_problem(s, n, d0, n_in)
    assert R.near_zero(X0, Wt0, b0) == 0
