"""The forward-only scaler path (`careless_amd.engine.scaler_forward`: what `scaler(inputs)`, the output step and the frozen-scaler step
run) on each of its three routes -- one fused launch, a chain of layer blocks, layer by layer in row chunks of whole images -- against
the fp64 oracle, with the launches counted, and in several row chunks against one.

The shapes are the smallest that take each route: 300 .. 600 rows = a ragged last tile of 128 and more than one chunk of 128 rows;
5 x 64 and 20 x 10 (the 64-wide and the lane kernel), 2 x 16 with two per-image layers (packed by image), 13 x 32 and 24 x 10 (one layer
more than a launch holds: two blocks), 2 x 96 (wider than a fused kernel), 2 x 72 and 12 x 32 with two per-image layers (grouped GEMMs),
2 x 136 with one (the tiled kernel above width 128), and 2 x 72 on images of 20, 0, 280 and 0 rows (an image longer than the chunk, empty
images in front of and behind a chunk).  scripts/trace_launches.py records the same cases argument by argument."""
import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

CASES = {
    "plain_5x64": dict(N=300, R=40, d0=5, L=5, w=64, S=1),
    "lane_20x10": dict(N=300, R=40, d0=5, L=20, w=10, S=1),
    "by_image_2x16_K2": dict(N=600, R=48, d0=5, L=2, w=16, S=2, n_images=4, image_layers=2),
    "chain_13x32": dict(N=500, R=40, d0=5, L=13, w=32, S=2),
    "chain_24x10": dict(N=300, R=30, d0=5, L=24, w=10, S=1),
    "wide_2x96": dict(N=300, R=40, d0=5, L=2, w=96, S=1),
    "wide_imgl_2x72_K2": dict(N=500, R=40, d0=5, L=2, w=72, S=2, n_images=5, image_layers=2),
    "wide_imgl_tiles_2x136_K1": dict(N=500, R=40, d0=5, L=2, w=136, S=1, n_images=3, image_layers=1),
    "deep_imgl_12x32_K2": dict(N=500, R=40, d0=5, L=12, w=32, S=1, n_images=5, image_layers=2),
    "unbalanced_imgl_2x72_K1": dict(N=300, n_images=4, w=72, L=2, image_layers=1),
}
UNBALANCED = "unbalanced_imgl_2x72_K1"
# entry point -> launches of ONE `scaler_forward` call in one row chunk
ONE_CHUNK = {
    "plain_5x64": {"cl_mlp_forward": 1}, "lane_20x10": {"cl_mlp_forward": 1}, "by_image_2x16_K2": {"cl_mlp_forward": 1},
    "chain_13x32": {"cl_mlp_forward": 2}, "chain_24x10": {"cl_mlp_forward": 2},
    "wide_2x96": {"cl_wide_dense_forward": 2, "cl_wide_head_forward": 1},
    "wide_imgl_2x72_K2": {"cl_wide_dense_forward": 2, "cl_wide_image_forward": 2, "cl_wide_head_forward": 1},
    "wide_imgl_tiles_2x136_K1": {"cl_wide_dense_forward": 2, "cl_wide_image_forward_tiles": 1, "cl_wide_head_forward": 1},
    "deep_imgl_12x32_K2": {"cl_wide_dense_forward": 12, "cl_wide_image_forward": 2, "cl_wide_head_forward": 1},
    UNBALANCED: {"cl_wide_dense_forward": 2, "cl_wide_image_forward": 1, "cl_wide_head_forward": 1},
}
CHUNK_128 = 0       # `engine.FORWARD_CHUNK_BYTES` below the formula's floor of 128 rows: chunks of 128 rows, or of whole images


def problem(name):
    """(data, cfg, params, x) of a case; the unbalanced one with its image ids rewritten: image 2 holds 280 rows, image 0 every
    fifteenth row (20 of them, scattered: the order by image moves them), images 1 and 3 none."""
    from oracle import elbo_oracle as O
    data, cfg, params, x, _, _ = util.make_problem(**CASES[name])
    if name == UNBALANCED:
        data = dict(data)
        data["image_id"] = np.where(np.arange(CASES[name]["N"]) % 15 == 7, 0, 2).astype(np.asarray(data["image_id"]).dtype)
        x = O.inputs_from_numpy(data)
    return data, cfg, params, x


def build(name):
    """(model, inputs, cfg, x, params) of a case."""
    data, cfg, params, x = problem(name)
    return util.build_model(data, cfg, params, CASES[name]["L"], CASES[name]["w"]), util.reference_inputs(data), cfg, x, params


def n_chunks(name):
    """Row chunks of the layer-by-layer route at the 128-row budget: `image_chunks` on the case's images, else ceil(N / 128)."""
    from careless_amd.obs import image_order
    from careless_amd.wide import image_chunks
    kw = CASES[name]
    if not kw.get("image_layers"):
        return -(-kw["N"] // 128)
    ids = np.asarray(problem(name)[0]["image_id"]).astype(np.int64)
    return len(image_chunks(image_order(ids, kw["n_images"])[1], 128))


@pytest.fixture
def launches(monkeypatch):
    """{entry point: calls} of every stream-taking entry point the test issues (tests/test_epilogue_plain.py wraps three this way)."""
    import ctypes as C

    from careless_amd import _lib
    lib, seen = _lib.get_lib(), {}
    for name, (res, argtypes) in _lib.EXPORTS.items():
        if argtypes and argtypes[-1] is C.c_void_p and res is C.c_int and not name.startswith("cl_host_"):
            def wrapped(*args, _name=name, _fn=getattr(lib, name)):
                seen[_name] = seen.get(_name, 0) + 1
                return _fn(*args)
            monkeypatch.setattr(lib, name, wrapped)
    return seen


@pytest.mark.parametrize("name", list(CASES))
def test_scaler_call_against_the_oracle_launch_counts_and_row_chunks(name, launches, monkeypatch):
    """`scaler(inputs)` at the default chunk budget (every case is one chunk), then at a budget of 128 rows: loc and scale against the
    oracle (the bound of the forward checks of tests/test_gpu_parity.py), the entry points and their counts -- the layer-by-layer
    counts times the number of chunks at 128 rows --, and the chunked outputs bit for bit the single-chunk ones (rows are independent,
    whole images stay together)."""
    import torch

    from careless_amd import engine
    from oracle import elbo_oracle as O
    model, inputs, cfg, x, params = build(name)
    imgl = dict(image_id=x.image_id, imgl_w=params.imgl_w, imgl_b=params.imgl_b) if CASES[name].get("image_layers") else {}
    o = O.mlp_forward(x.metadata, params.mlp_w, params.mlp_b, cfg.leakiness, **imgl)
    want_loc, want_scale = o[:, 0].numpy(), O.scale_bijector(o[:, 1], "exp", cfg.epsilon).numpy()
    wide = "cl_wide_head_forward" in ONE_CHUNK[name]
    outs = []
    for budget, chunks in ((None, 1), (CHUNK_128, n_chunks(name) if wide else 1)):
        if budget is not None:
            monkeypatch.setattr(engine, "FORWARD_CHUNK_BYTES", budget)
        launches.clear()
        dist = model.scaling_model(inputs)
        torch.cuda.synchronize()
        loc, scale = dist.loc.cpu().numpy(), dist.scale.cpu().numpy()
        e_loc, e_scale = util.rel_err(loc, want_loc), util.rel_err(scale, want_scale)
        print(f"{name}: budget {budget} chunks {chunks} rel err loc {e_loc:.2e} scale {e_scale:.2e} launches {dict(launches)}")
        assert e_loc < 1e-5 and e_scale < 1e-5
        assert dict(launches) == {k: v * chunks for k, v in ONE_CHUNK[name].items()}
        outs.append((loc, scale))
    assert chunks > 1 or not wide
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
