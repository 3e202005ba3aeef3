"""The index arithmetic of the frozen-scaler data term (careless_amd/frozen.py) on CPU tensors, against a restatement in plain Python
loops.  (The argument checks of `cl_frozen_rows`: tests/test_host_logic.py.)"""
import numpy as np
import pytest
import torch

from careless_amd.frozen import group_row_order, sorted_row_order

def _stable_by(ids, rows):
    return sorted(rows, key=lambda i: (ids[i], i))


def _mono_ids():
    """130 rows (two full waves and a tail) whose reflection runs, once sorted, cross rows 63 / 64 and 127 / 128; reflection 2 has a
    single row, reflection 3 none."""
    rid = np.repeat([0, 1, 2, 4, 5], [60, 10, 1, 49, 10])
    assert len(rid) == 130 and rid[63] == rid[64] == 1 and rid[127] == rid[128] == 5
    return np.random.default_rng(5).permutation(rid).astype(np.int32)


@pytest.mark.parametrize("start", [0, 1000])
@pytest.mark.parametrize("shuffled_index", [False, True])
def test_sorted_row_order(start, shuffled_index):
    rid = _mono_ids()
    N = len(rid)
    rows = np.random.default_rng(6).permutation(5000)[:N].astype(np.int64) if shuffled_index else None
    order, key = sorted_row_order(torch.as_tensor(rid), start, None if rows is None else torch.as_tensor(rows))
    want = _stable_by(rid, range(N))
    assert order.tolist() == want and key.dtype == torch.int32 and key.is_contiguous()
    assert key.tolist() == [int(rows[i]) if rows is not None else start + i for i in want]       # key = the global row of every sorted row
    srt = rid[order.numpy()]
    assert all(srt[i] < srt[i + 1] or (srt[i] == srt[i + 1] and want[i] < want[i + 1]) for i in range(N - 1))     # ascending, ties in row order


@pytest.mark.parametrize("with_noise_row", [False, True])
def test_group_row_order(with_noise_row):
    n_pad, N, start = 256, 200, 1000
    rng = np.random.default_rng(7)
    row_map = np.full(n_pad, -1, dtype=np.int32)
    row_map[np.sort(rng.permutation(n_pad)[:N])] = rng.permutation(N)              # 56 padding positions mixed in
    rid = np.where(row_map >= 0, rng.integers(0, 12, n_pad), -1).astype(np.int32)
    rid[np.nonzero(row_map >= 0)[0][::9]] = -1                                     # rows that have no reflection
    noise = rng.permutation(9000)[:n_pad].astype(np.int32) if with_noise_row else None
    rmc, key, src, dst, refl_sorted, n2 = group_row_order(torch.as_tensor(rid), torch.as_tensor(row_map), start,
                                                           None if noise is None else torch.as_tensor(noise))
    active = [i for i in range(n_pad) if row_map[i] >= 0 and rid[i] >= 0]
    want_src = _stable_by(rid, active)
    assert 0 < len(active) < N and n2 == len(active) and src.tolist() == want_src
    assert rmc.tolist() == [max(int(r), 0) for r in row_map] and rmc.dtype == torch.int64
    assert key.dtype == torch.int32 and key.tolist() == ([int(k) for k in noise] if with_noise_row else [start + max(int(r), 0) for r in row_map])
    assert refl_sorted.dtype == torch.int32 and refl_sorted.tolist() == [int(rid[i]) for i in want_src]
    assert all(a < b or (a == b and i < j) for a, b, i, j in zip(refl_sorted.tolist(), refl_sorted.tolist()[1:], want_src, want_src[1:]))
    assert dst.dtype == torch.int32 and dst[src].tolist() == list(range(n2))
    rest = np.ones(n_pad, dtype=bool)
    rest[want_src] = False
    assert (dst.numpy()[rest] == -1).all()


def test_row_keys_are_bounded_by_int32():
    """The kernels read a row's noise key as int32: the largest key 2^31 - 1 passes, 2^31 raises (N = 130: nothing large is allocated)."""
    rid = torch.as_tensor(_mono_ids())
    N, top = len(rid), 1 << 31
    assert int(sorted_row_order(rid, top - N)[1].max()) == top - 1
    with pytest.raises(ValueError, match="shard the data further"):
        sorted_row_order(rid, top - N + 1)
    rows = torch.arange(N, dtype=torch.int64) * 3
    rows[17] = top - 1
    assert int(sorted_row_order(rid, 0, rows)[1].max()) == top - 1
    rows[17] = top
    with pytest.raises(ValueError, match="shard the data further"):
        sorted_row_order(rid, 0, rows)
    row_map = torch.full((256,), -1, dtype=torch.int32)
    row_map[50:50 + N] = torch.arange(N, dtype=torch.int32)
    gid = torch.where(row_map >= 0, 1, -1).to(torch.int32)
    assert int(group_row_order(gid, row_map, top - N)[1].max()) == top - 1
    with pytest.raises(ValueError, match="shard the data further"):
        group_row_order(gid, row_map, top - N + 1)
