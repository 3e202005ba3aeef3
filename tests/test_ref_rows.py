"""tests/ref_rows.py checked without a GPU: the fp64 reference of the row-level data-term kernels against the oracle's whole step with the
scaler replaced by the given (loc, sigma), its summand sizes, the fp32 emulation of the kernels (numpy float32 in the kernels' order of
operations and of sums, scalar functions from the host build of csrc/cl_math.h) inside a quarter of every bound of
tests/test_rows_kernels_gpu.py on the inputs of every GPU case, and wrong kernels ("mutants" of the emulation) each outside a bound by 4 x
or more on some GPU case's inputs.

A quarter of a gradient bound: the kernel's own share, RTOL_GRAD M, is held to a quarter; the rounding of the store (u |stored value|, the
bound's second term) is used up to the full by ANY kernel and is allowed in full (ref_rows._worst_grad, as ref_q._worst_grad).

Measured here (host build, glibc's expf / logf / log1pf), the largest ratio to each bound over the GPU cases' inputs (printed with -s):
    cl_frozen_rows ROWS       dz_f wide 4.0e-3, fitted 1.3e-3; max-norm 5.1e-3; ipred 2.4e-3; NLL 9.5e-4; d_ev11 4.3e-4
    cl_frozen_rows GROUPS     gbuf wide 0.14, fitted 0.071; gbuf max-norm 8.6e-3; dz_f after SUMS 1.9e-3, max-norm 1.2e-2; NLL 1.1e-3; d_ev11 2.4e-3
    cl_laue_*                 iconv 6.0e-3; dNLL/diconv 5.4e-3; dz_f 5.2e-3; dO 5.1e-3; d_img 1.8e-3; d_ev11 9e-4; NLL 9.3e-4; max-norms <= 2.6e-3
    cl_slot_rows              dz_f wide 1.8e-2, fitted 8.6e-3; dO 6.1e-3, max-norm 7.4e-2; d_img 4.0e-3; NLL 1.1e-3
    cl_det_reduce             0 on the dyadic inputs, 0.49 of the a-priori fp32 bound on floats
The bars are the project's parity tolerances, two to three decades above fp32 rounding: the quarter is met with room everywhere.
Mutants, the factor by which each misses a bound on some GPU case's inputs:
    chain_stops_after_one_wave 4.8e3   first_cp_ignored 4.8e3   rec1_total_to_dzf 4.4e3   no_aim_in_dzf 1.1e4   z_not_2z 2.5e3   no_w_ll 6.8e4
    eta_by_sorted_position 2.3e5   every_member_counts_nll 2.9e4   group_sum_over_gmax 4.8e10   padded_slots_not_counted 9.7e3
    harmonic_id_ignored_in_backward 3.9e13   second_head_dO_dropped 5.0e3   image_0_has_a_gradient 1.1e6   no_lane_by_lane_tail 5.0e3
    det_slot_not_times_S inf (a record lands on an entry whose summand size is zero)
    cl_det_reduce: first_pass_only 3.5e14   store_not_add 1.0e15
    rid_after_at_lane_63: no VALUE moves (every bound at 1.9e-3, the unmutated figure); outside the exact bar on the edge records.  With
    rid_after read at row0 + 63, last_cn holds for every full wave: the wave's last run goes to edge record 1 and the edge launch stores it
    -- its walk stops at the next wave, whose first_cp comes from rid_before and is false; a through-wave gets the THROUGH flag and the walk
    stops one wave later for the same reason.  Every total is the same sum in the same order; what differs is which launch stores it, and
    the records in edge_rid, which the layout fixes and ref_rows.rows_ratios compares exactly (here and on the device).
"""
import numpy as np
import pytest
import torch

from oracle import elbo_oracle as O
from tests import ref_rows as RR
from tests import ref_step

T = RR.T


@pytest.fixture(scope="module")
def hm():
    lib = RR.host_lib()
    if lib is None:
        pytest.skip("g++ not available")
    return lib


def test_tolerances_are_the_projects_own():
    from tests import test_gpu_parity as P
    assert (RR.RTOL_LOSS, RR.RTOL_GRAD) == (P.RTOL_LOSS, P.RTOL_GRAD) and RR.U == ref_step.U


# ---- a. the reference against the oracle -------------------------------------------------------------------------------------------------------
def _oracle_problem(laue, kind, ev11, seed):
    """A small problem whose scaler IS the given (loc, sigma): no hidden layer, metadata = (loc, log(sigma - eps)), an identity output layer and
    the exp bijector, so that O.elbo_forward's scaler returns exactly them."""
    rng = np.random.default_rng([41, int(laue), RR.KINDS[kind], int(ev11), seed])
    n, R, S, M, eps, shift = 60, 9, 3, 5, 1e-7, 0.37
    x = type("X", (), {})()
    x.n, x.R, x.S, x.kind, x.dof, x.shift, x.w_ll = n, R, S, kind, 6.5, shift, 1.0 / S
    x.refl_id = rng.integers(0, R, n).astype(np.int32)
    x.image_id = np.sort(rng.integers(0, M, n)).astype(np.int32)
    x.img, x.aim = rng.uniform(0.5, 2.0, M - 1), None
    x.loc = rng.normal(2.0, 1.0, n)
    raw = np.log(rng.uniform(0.05, 0.5, n))
    x.sigma = (torch.exp(T(raw)) + eps).numpy()
    x.iobs, x.sig = rng.uniform(0.0, 30.0, n), rng.uniform(0.3, 3.0, n)
    x.eta_row = rng.standard_normal((n, S))
    x.ev11 = np.array(RR.EV11_RAW, np.float64) if ev11 else None
    if laue:
        G = 37                                                                       # G < n: the slots G .. n - 1 keep iconv = 0 and count
        x.slot = rng.integers(0, G, n)
        x.slot[:G] = rng.permutation(G)
    else:
        x.slot = None
    x.count = np.ones(n, bool)
    cfg = O.ElboConfig(mc_samples=S, likelihood=kind, dof=x.dof, scale_bijector="exp", epsilon=eps, scale_shift=shift,
                       use_image_scales=True, laue=laue, ev11=ev11)
    p = O.ElboParams(T(rng.normal(0.0, 0.3, R)), T(np.log(rng.uniform(0.05, 0.3, R))), [torch.eye(2, dtype=torch.float64)], [torch.zeros(2, dtype=torch.float64)],
                     img_raw=T(x.img), ev11_raw=T(x.ev11) if ev11 else None)
    inp = O.ElboInputs(torch.as_tensor(x.refl_id.astype(np.int64)), torch.as_tensor(x.image_id.astype(np.int64)), T(np.stack([x.loc, raw], 1)), T(x.iobs), T(x.sig),
                       torch.zeros(R, dtype=torch.bool), T(np.ones(R)), T(np.full(R, 1e-32)), sigma=T(1.0),
                       harmonic_id=torch.as_tensor(x.slot.astype(np.int64)) if laue else None)
    u_f = T(rng.uniform(0.05, 0.95, (S, R)))
    return x, cfg, p, inp, u_f, raw, eps


@pytest.mark.parametrize("laue", [False, True], ids=["mono", "laue"])
@pytest.mark.parametrize("kind,ev11", [("normal", False), ("normal", True), ("studentt", False), ("studentt", True), ("laplace", False)])
def test_reference_equals_the_oracle_with_the_scaler_replaced(laue, kind, ev11):
    """ipred, NLL and every gradient the kernels write against O.elbo_value_and_grads (the image scales and the Evans-2011 triple: the KL does
    not depend on them) and against autograd through O.elbo_forward's own graph (dz_f, d / d(loc, sigma)), at 1e-12 of the summand size; the
    summand sizes dominate every entry."""
    for seed in (0, 1):
        x, cfg, p, inp, u_f, raw, eps = _oracle_problem(laue, kind, ev11, seed)
        eta = T(x.eta_row.T)
        lap = kind == "laplace"
        out, grads = O.elbo_value_and_grads(p, inp, cfg, u_f, eta)
        x.z_f = out["z_f"].numpy().T.copy()
        ref = RR.reference(x)
        assert np.all(np.abs(ref.ipred - out["ipred"].numpy().T) <= 1e-12 * ref.M_ipred)
        assert abs(ref.nll - float(out["nll"])) <= 1e-12 * ref.M_nll
        g_img = grads[4]
        assert np.all(np.abs(ref.d_img - g_img.numpy()) <= 1e-12 * ref.M_img)
        if ev11:
            assert np.all(np.abs(ref.d_ev11 - grads[5].numpy()) <= 1e-12 * ref.M_ev11) and np.all(ref.M_ev11 >= np.abs(ref.d_ev11))
        if not lap:                                                   # dz_f and dO through the oracle's own graph
            q = p.clone(requires_grad=True)
            meta = inp.metadata.clone().requires_grad_(True)
            inp2 = O.ElboInputs(**{**inp.__dict__, "metadata": meta})
            fw = O.elbo_forward(q, inp2, cfg, u_f, eta)
            dz, dm = torch.autograd.grad(fw["nll"], [fw["z_f"], meta])
            assert np.all(np.abs(ref.dz - dz.numpy().T) <= 1e-12 * ref.M_dz)
            dO = np.stack([dm[:, 0].numpy(), dm[:, 1].numpy() / np.exp(raw)], 1)
            assert np.all(np.abs(ref.dO - dO) <= 1e-12 * ref.M_dO)
        for v, M in ((ref.ipred, ref.M_ipred), (ref.iconv, ref.M_iconv), (ref.dz, ref.M_dz), (ref.dO, ref.M_dO), (ref.d_img, ref.M_img), (ref.dconv, ref.M_dconv),
                     (ref.gbuf, ref.M_gbuf)):
            assert np.all(M * (1.0 + 1e-12) >= np.abs(v)), (laue, kind, ev11)
        assert ref.M_nll * (1.0 + 1e-12) >= abs(ref.nll)
        # the rows' own shares add up to dz_f; a row without a reflection contributes nothing; image 0 has no gradient
        tot = np.zeros_like(ref.dz)
        np.add.at(tot, x.refl_id, ref.gbuf)
        assert np.all(np.abs(tot - ref.dz) <= 1e-12 * ref.M_dz)
        if laue:
            empty = np.bincount(x.slot, minlength=x.n) == 0
            assert empty.sum() >= x.n - 37 and np.all(ref.iconv[empty] == 0.0) and np.all(ref.M_dconv[empty] > 0.0)
        x.refl_id = x.refl_id.copy()
        x.refl_id[:5] = -1
        if not laue:
            x.count = x.refl_id >= 0
            off = RR.reference(x)
            assert np.all(off.ipred[:5] == 0.0) and np.all(off.dO[:5] == 0.0) and np.all(off.M_gbuf[:5] == 0.0) and abs(off.nll) < abs(ref.nll)


# ---- d. what the case list covers ----------------------------------------------------------------------------------------------------------------
def test_case_list_covers_what_the_kernels_branch_on():
    cs = RR.GPU_CASES
    rows = [c for c in cs if c.entry == "rows"]
    assert {c.layout for c in rows} == set(RR.ROW_LAYOUTS) and {c.S for c in rows} == set(RR.ROWS_S)
    feats = {name: RR.rows_features(RR.runs_layout(**kw)[0]) for name, kw in RR.ROW_LAYOUTS.items()}
    want = {"run of one row", "run ends at lane 63, next starts at lane 0", "run crosses a wave border", "through-wave", "through-wave at a chunk border",
            "run starts at lane 0, fills its wave and goes on", "two chains back to back", "chain ends in the ragged last wave", "R = 1",
            "a whole wave without a reflection", "refl_id < 0 ends mid-wave", "above the grid cap"}
    assert set().union(*feats.values()) == want
    for name, f in (("lane63", "run ends at lane 63, next starts at lane 0"), ("through", "through-wave at a chunk border"), ("lane0full", "run starts at lane 0, fills its wave and goes on"),
                    ("back2back", "two chains back to back"), ("raggedend", "chain ends in the ragged last wave"), ("big", "above the grid cap")):
        assert f in feats[name], (name, feats[name])
    assert "run crosses a wave border" not in feats["lane63"] and "run crosses a wave border" not in feats["ones"]
    assert {len(RR.runs_layout(**RR.ROW_LAYOUTS[k])[0]) for k in ("n1", "n63", "n64", "n65", "n256", "n257", "n641")} == {1, 63, 64, 65, 256, 257, 641}
    assert len(RR.runs_layout(**RR.ROW_LAYOUTS["big"])[0]) == RR.N_BIG > RR.CAP * RR.FB and max(RR.ROW_LAYOUTS["big"]["runs"]) == 70000
    for name, kw in RR.ROW_LAYOUTS.items():                           # reflections without rows, R - 1 among them
        rid, R = RR.runs_layout(**kw)
        assert np.all(np.diff(rid) >= 0) and rid.max() < R
    assert any(RR.runs_layout(**kw)[1] - 1 > RR.runs_layout(**kw)[0].max() for kw in RR.ROW_LAYOUTS.values())
    chains = [c for c in rows if "run crosses a wave border" in feats[c.layout] and c.layout != "big"]
    for opt, values in (("aim", {True, False}), ("key", {True, False}), ("accumulate", {0, 1}), ("nll", {"atomic", "part"}), ("ipred_out", {True, False}),
                        ("kind", {"normal", "studentt", "laplace"}), ("ev11", {None, "atomic", "part"}), ("family", {"wide", "fitted"})):
        assert {getattr(c, opt) for c in chains} == values, opt        # every option crossed with a chain layout
    assert {c.S for c in chains} == set(RR.ROWS_S) and {c.S for c in rows if c.layout == "big"} == {1, 8}
    grp = [c for c in cs if c.entry == "groups"]
    assert {c.layout for c in grp} == set(RR.GROUPS_N2) and {c.S for c in grp} == set(RR.GROUPS_S) and {c.src for c in grp} == {True, False}
    assert {c.kind for c in grp} == {"normal", "studentt", "laplace"} and {c.ev11 for c in grp} == {None, "atomic", "part"}
    for n2 in RR.GROUPS_N2:
        refl, gmeta, start, R = RR.groups_layout(n2, 0)
        act = refl >= 0
        size, mem = gmeta >> 8, gmeta & 0xff
        assert act.sum() == n2 and len(refl) % 16 == 0 and (n2 < 600 or len(refl) % 256 != 0)
        assert set(size[act]) == ({1, 2, 3, 5, 16} if n2 > 100 else set(size[act])) and np.all((start[act] // 16) == ((start[act] + size[act] - 1) // 16))
        assert np.all(np.arange(len(refl))[act] == start[act] + mem[act]) and np.any(~act) and refl[act].max() < R - 1
    # cl_det_reduce
    ds = RR.DET_CASES
    assert {c.S for c in ds} == set(RR.DET_S) and {c.R for c in ds} == set(RR.DET_R) and {c.nparts for c in ds} == set(RR.DET_NPARTS)
    assert {c.n_ev11 for c in ds} == set(RR.DET_NEV) and {c.n_images for c in ds} == set(RR.DET_IMAGES) and {c.perm for c in ds} == {True, False}
    assert {c.dyadic for c in ds} == {True, False} and any(not c.d_img for c in ds)
    x = RR.det_inputs(next(c for c in ds if c.R == 1100))
    assert set(np.diff(x.seg_refl)) == set(RR.DET_REFL_ROWS)
    x = RR.det_inputs(next(c for c in ds if c.n_images == 6))
    assert set(np.diff(x.seg_img)[1:]) == set(RR.DET_IMG_ROWS)


def test_group_layout_by_hand_is_what_pack_laue_builds():
    """The packed order the GROUPS cases build from the header's contract against obs.pack_laue on the same groups: a group inside a granule,
    gmeta = member | size << 8, the members of a group consecutive."""
    from careless_amd import obs
    refl, gmeta, start, R = RR.groups_layout(641, 0)
    act = np.flatnonzero(refl >= 0)
    hid = start[act]                                                   # one harmonic id per group
    pos, n_pad, gm, tile_gmax, row_map, tile_img = obs.pack_laue(hid, np.zeros(len(act), np.int64), False)
    assert np.array_equal(gm[pos], gmeta[act])                         # member index and size of every row
    assert np.all(pos // 16 == (pos - (gm[pos] & 0xff) + (gm[pos] >> 8) - 1) // 16) and np.all(row_map[pos] == np.arange(len(act)))
    assert np.all(gm[row_map < 0] == 0) and np.all(gmeta[refl < 0] == 0)


# ---- b. the fp32 emulation inside a quarter of every bound ----------------------------------------------------------------------------------------
MEASURED = {}


@pytest.mark.parametrize("c", RR.GPU_CASES, ids=lambda c: c.id)
def test_emulation_stays_inside_a_quarter_of_every_bound(hm, c):
    x, ref = RR.reference_for(c)
    r = RR.rows_ratios(x, ref, RR.emulate(x, hm))
    print(c.id, {k: f"{v:.2e}" for k, v in sorted(r.items())})
    for k, v in r.items():
        key = (c.entry, c.family, k)
        MEASURED[key] = max(MEASURED.get(key, 0.0), v)
        assert v <= 0.25, (c.id, k, v)


# ---- c. mutants -----------------------------------------------------------------------------------------------------------------------------------
CHAIN3 = lambda c: c.entry == "rows" and c.layout in ("through", "big", "n641") and not c.accumulate
TARGETS = {
    "chain_stops_after_one_wave": CHAIN3,
    "first_cp_ignored": lambda c: c.entry == "rows" and c.layout in ("cross1", "through", "back2back") and not c.accumulate,
    "rid_after_at_lane_63": lambda c: c.entry == "rows" and c.layout in ("lane63", "cross1", "through", "back2back", "lane0full", "n641"),
    "rec1_total_to_dzf": lambda c: c.entry == "rows" and c.layout in ("cross1", "through", "back2back") and not c.accumulate,
    "no_aim_in_dzf": lambda c: c.entry == "rows" and c.aim,
    "z_not_2z": lambda c: c.entry == "rows",
    "no_w_ll": lambda c: c.entry == "rows" and c.S > 1,
    "eta_by_sorted_position": lambda c: c.entry == "rows" and c.key and c.layout != "big",
    "every_member_counts_nll": lambda c: c.entry == "groups",
    "group_sum_over_gmax": lambda c: c.entry == "groups",
}


@pytest.mark.parametrize("mutant", RR.ROWS_MUTANTS + RR.GROUPS_MUTANTS)
def test_every_mutant_is_outside_a_bound_by_four_times(hm, mutant):
    cases = [c for c in RR.GPU_CASES if TARGETS[mutant](c)][:6]
    assert cases
    best = (0.0, None, None)
    for c in cases:
        x, ref = RR.reference_for(c)
        r = RR.rows_ratios(x, ref, RR.emulate(x, hm, mutant=mutant))
        k = max(r, key=r.get)
        best = max(best, (r[k], k, c.id))
    print(mutant, best)
    assert best[0] >= 4.0, (mutant, best)


# ---- cl_det_reduce ----------------------------------------------------------------------------------------------------------------------------------
def test_det_reduce_emulation_and_its_mutants():
    worst, mut = 0.0, {m: 0.0 for m in RR.DET_MUTANTS}
    for c in RR.DET_CASES:
        x = RR.det_inputs(c)
        ref = RR.det_reference(x)
        r = RR.det_ratios(x, ref, RR.emulate_det(x))
        if c.dyadic:
            assert all(v == 0.0 for v in r.values()), (c.id, r)       # (the grid: every fp32 sum is exact)
        else:
            assert all(v <= 1.0 for v in r.values()), (c.id, r)       # (a-priori: a lone rounding reaches it)
            worst = max(worst, max(r.values()))
        for m in RR.DET_MUTANTS:
            if m == "first_pass_only" and not np.any(np.diff(x.seg_refl) > 16):
                continue
            mut[m] = max(mut[m], RR.det_ratios(x, ref, RR.emulate_det(x, mutant=m))["dz_f"])
    print("cl_det_reduce, floats: error / a-priori fp32 bound", worst, "mutants", mut)
    assert all(v >= 4.0 for v in mut.values()), mut


# ---- rows in the caller's order: the three Laue calls and cl_slot_rows ---------------------------------------------------------------------------
def test_laue_and_slot_case_list_covers_what_the_kernels_branch_on():
    cs = RR.LGPU_CASES
    laue, slot = [c for c in cs if c.entry == "laue"], [c for c in cs if c.entry == "slot"]
    assert {c.S for c in laue} == set(RR.LAUE_S) and {c.S for c in slot} == set(RR.SLOT_S)
    assert {c.kind for c in laue} == {c.kind for c in slot} == {"normal", "studentt", "laplace"} and {c.ev11 for c in laue} == {None, "atomic", "part"}
    assert {c.dO for c in laue} == {True, False} and any(c.img_run == 0 for c in laue) and any(c.img_run == 0 for c in slot)
    assert any(c.n * c.S > RR.PAIRS_CAP for c in laue)                                 # the likelihood's grid-stride loop
    rounds = {-(-c.n * c.S // RR.PAIRS_CAP) for c in slot}
    assert rounds == {1, 2, 3}                                                         # one round, a pair of rounds, a last odd round on an inactive pair
    assert {c.S for c in slot if c.det and not c.det_slot} == {1, 4, 16, 64} and {c.S for c in slot if c.det_slot} == {1, 4, 8, 16, 64}
    assert any(c.det_slot and c.n * c.S > RR.PAIRS_CAP for c in slot)                  # the scattered stores in a second round of the loop
    x = RR.make_linputs(next(c for c in slot if c.det_slot and c.S == 4))
    assert x.perm_refl is None and x.seg_refl[0] == RR.DET_LEAD and x.seg_refl[-1] == RR.DET_LEAD + x.n
    assert np.array_equal(np.sort(x.det_slot), RR.DET_LEAD + np.arange(x.n)) and np.all(np.diff(x.refl_id[np.argsort(x.det_slot)]) >= 0)
    for c in cs:                                                                       # images per wave: one, two to four, more than four
        if c.img_run:
            per = (64 // c.S) / c.img_run if c.S <= 64 else 0
            c.images_per_wave = "one" if per <= 0.1 else ("few" if per <= 3 else "many")
    for sub in (laue, slot):
        assert {getattr(c, "images_per_wave", None) for c in sub if c.img_run} >= {"one", "few", "many"}
    x = RR.make_linputs(next(c for c in laue if c.S == 3))
    sizes = np.bincount(x.slot, minlength=x.n)
    assert x.G < x.n and sizes.max() == 40 and sizes[x.G:].max() == 0 and sizes[:x.G].min() >= 1 and np.any(np.diff(x.slot) < 0)
    assert x.image_id.min() == 0 and not x.has_rows[-1]


@pytest.mark.parametrize("c", RR.LGPU_CASES, ids=lambda c: c.id)
def test_laue_and_slot_emulation_stays_inside_a_quarter_of_every_bound(hm, c):
    x, ref = RR.lreference_for(c)
    r = RR.laue_ratios(x, ref, RR.lemulate(x, hm))
    print(c.id, {k: f"{v:.2e}" for k, v in sorted(r.items())})
    for k, v in r.items():
        key = (c.entry, c.family, k)
        MEASURED[key] = max(MEASURED.get(key, 0.0), v)
        assert v <= 0.25, (c.id, k, v)


LTARGETS = {
    "padded_slots_not_counted": lambda c: c.entry == "laue",
    "harmonic_id_ignored_in_backward": lambda c: c.entry == "laue",
    "second_head_dO_dropped": lambda c: c.entry == "slot" and 64 % c.S != 0 and not c.det,
    "image_0_has_a_gradient": lambda c: c.entry == "slot" and c.img_run and not c.det and c.n < 1000,
    "no_lane_by_lane_tail": lambda c: c.entry == "slot" and c.img_run and not c.det and (64 // c.S) / c.img_run > 4,
    "det_slot_not_times_S": lambda c: c.entry == "slot" and c.det_slot and c.S > 1 and c.n < 1000,
}


@pytest.mark.parametrize("mutant", RR.LAUE_MUTANTS + RR.SLOT_MUTANTS)
def test_every_laue_and_slot_mutant_is_outside_a_bound_by_four_times(hm, mutant):
    cases = [c for c in RR.LGPU_CASES if LTARGETS[mutant](c)][:6]
    assert cases
    best = (0.0, None, None)
    for c in cases:
        x, ref = RR.lreference_for(c)
        r = RR.laue_ratios(x, ref, RR.lemulate(x, hm, mutant=mutant))
        k = max(r, key=r.get)
        best = max(best, (r[k], k, c.id))
    print(mutant, best)
    assert best[0] >= 4.0, (mutant, best)


def test_report_the_measured_fractions():
    """(printed with -s: the figures of the module docstring)"""
    print({" ".join(k): f"{v:.2e}" for k, v in sorted(MEASURED.items())})
