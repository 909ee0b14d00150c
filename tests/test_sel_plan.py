"""Selection planning (plan.sel_normalize / compose / sel_plan) — pure
Python, no device.  Every expected value comes from numpy indexing of a
host array; sel_plan is EXECUTED here on per-chunk numpy arrays (gather
each piece with np.ix_, place it at its positions) and compared with
full[np.ix_(...)], with a write count so a dropped or doubled piece
cannot pass."""
import numpy as np
import pytest

from distributedarrays_jl_amd import plan
from distributedarrays_jl_amd._ffi import DArrayError


def _ix(sel):
    return np.ix_(*[plan.sel_indices(e) for e in sel])


# ------------------------------------------------------------ normalise
@pytest.mark.parametrize("sub", [
    slice(None), slice(None, None, 3), slice(None, None, -1),
    slice(5, None, -2), slice(2, 17, 4), slice(30, 2, -7), slice(7, 7),
    slice(-5, None), slice(None, -3, 2), slice(100, 200), slice(3, 1),
    [7, 0, 7, 39], [], np.array([4, 4, 1]), range(3, 30, 5),
])
def test_normalize_1d_matches_numpy(sub):
    a = np.arange(40) * 10
    sel, squeeze = plan.sel_normalize((sub,), (40,))
    assert squeeze == ()
    ref = a[list(sub)] if isinstance(sub, range) else \
        a[np.asarray(sub, dtype=np.int64)] if isinstance(sub, list) else a[sub]
    assert np.array_equal(a[_ix(sel)], ref)
    assert plan.sel_shape(sel) == ref.shape


def test_normalize_mixed_outer_product_and_squeeze():
    m = np.arange(6 * 7 * 5).reshape(6, 7, 5)
    sel, squeeze = plan.sel_normalize((slice(None, None, 2), 1,
                                       [4, 0, 0]), m.shape)
    assert squeeze == (1,)
    assert plan.sel_shape(sel) == (3, 1, 3)
    got = m[_ix(sel)].squeeze(axis=squeeze)
    # outer product (Julia), not numpy's zipped fancy indexing
    assert np.array_equal(got, m[::2, 1, :][:, [4, 0, 0]])
    sel2, _ = plan.sel_normalize(([0, 2], [1, 3]), (4, 4))
    m2 = np.arange(16).reshape(4, 4)
    assert np.array_equal(m2[_ix(sel2)], m2[np.ix_([0, 2], [1, 3])])
    assert m2[_ix(sel2)].shape == (2, 2)


@pytest.mark.parametrize("subs,dims", [
    ((40,), (40,)), ((-1,), (40,)), (([0, 40],), (40,)), (([-1],), (40,)),
    ((1, 2), (40,)), (([1.5],), (40,)), (([[1, 2]],), (40,)),
    ((np.array([True, False]),), (2,)), (("x",), (4,)),
])
def test_normalize_rejects(subs, dims):
    with pytest.raises(DArrayError):
        plan.sel_normalize(subs, dims)


# -------------------------------------------------------------- compose
def test_compose_matches_numpy_view_of_view():
    rng = np.random.default_rng(11)
    for _ in range(100):
        nd = int(rng.integers(1, 4))
        dims = tuple(int(rng.integers(1, 12)) for _ in range(nd))
        a = np.arange(int(np.prod(dims))).reshape(dims)
        outer = _rand_sel(rng, dims)
        inner = _rand_sel(rng, plan.sel_shape(outer))
        both = plan.compose(outer, inner)
        assert np.array_equal(a[_ix(both)], a[_ix(outer)][_ix(inner)])
    with pytest.raises(DArrayError):
        plan.compose((("a", 0, 1, 3),), (("a", 0, 1, 4),))


def test_expand_and_duplicates():
    sel = (("a", 1, 2, 3), ("v", np.array([1, 0])))
    full = plan.sel_expand(sel, 4, (0, 2))
    assert plan.sel_shape(full) == (1, 3, 1, 2)
    with pytest.raises(DArrayError):
        plan.sel_expand(sel, 2, (0,))
    assert not plan.sel_has_duplicates(sel)
    assert plan.sel_has_duplicates((("v", np.array([3, 1, 3])),))


# ------------------------------------------------------------- sel_plan
def _rand_sub(rng, n):
    """One random subscript entry over a dimension of length n."""
    kind = int(rng.integers(0, 6))
    if n == 0 or kind == 0:
        return ("a", 0, 1, n)                        # full / empty dim
    if kind == 1:                                    # empty selection
        return ("a", 0, 1, 0) if rng.integers(0, 2) else \
            ("v", np.zeros(0, dtype=np.int64))
    if kind in (2, 3):                               # stepped, both signs
        step = int(rng.integers(1, n + 3))           # incl. > chunk / dim
        if kind == 3:
            step = -step
        start = int(rng.integers(0, n))
        r = range(start, n if step > 0 else -1, step)
        cnt = int(rng.integers(1, len(r) + 1))
        return ("a", start, step, cnt)
    if kind == 4:                                    # unsorted + repeats
        return ("v", rng.integers(0, n, int(rng.integers(1, 2 * n + 2)))
                .astype(np.int64))
    return ("a", int(rng.integers(0, n)), 1, 1)      # an int subscript


def _rand_sel(rng, dims):
    return tuple(_rand_sub(rng, n) for n in dims)


def _rand_cuts(rng, n, k):
    """k ragged chunks of [0, n), empties allowed."""
    c = np.sort(rng.integers(0, n + 1, k - 1))
    edges = [0] + [int(x) for x in c] + [n]
    return [(edges[i], edges[i + 1]) for i in range(k)]


def _layout(rng, dims, world):
    """Random chunk boxes over `dims`: a grid of at most `world` chunks
    with ragged cuts, owners a random injective rank assignment."""
    nd = len(dims)
    while True:
        grid = [int(rng.integers(1, world + 1)) for _ in range(nd)]
        if int(np.prod(grid)) <= world:
            break
    per_dim = [_rand_cuts(rng, dims[d], grid[d]) for d in range(nd)]
    idxs = []
    for lin in range(int(np.prod(grid))):
        rem, box = lin, []
        for d in range(nd):
            box.append(per_dim[d][rem % grid[d]])
            rem //= grid[d]
        idxs.append(tuple(box))
    ranks = [int(r) for r in rng.permutation(world)[:len(idxs)]]
    return idxs, ranks


def _execute(full, idxs, ranks, sels_all):
    """Run the plan on numpy chunks; returns per-rank (result, writes)."""
    chunks = {ranks[c]: full[tuple(slice(lo, hi) for lo, hi in idx)]
              for c, idx in enumerate(idxs)}
    outs = {}
    for r, sel in enumerate(sels_all):
        if sel is not None:
            shp = plan.sel_shape(sel)
            outs[r] = (np.full(shp, -1, dtype=full.dtype),
                       np.zeros(shp, dtype=np.int64))
    pieces = plan.sel_plan(idxs, ranks, sels_all)
    keys = [(p[0], p[1]) for p in pieces]
    assert keys == sorted(keys), "pieces must be sorted by (src, dst)"
    for src, dst, lsel, psel in pieces:
        assert plan.sel_shape(lsel) == plan.sel_shape(psel)
        assert all(n > 0 for n in plan.sel_shape(lsel)), "empty piece kept"
        assert not plan.sel_has_duplicates(psel)
        block = chunks[src][_ix(lsel)]
        res, writes = outs[dst]
        res[_ix(psel)] = block
        writes[_ix(psel)] += 1
    return outs


def test_sel_plan_sweep():
    rng = np.random.default_rng(20261020)
    ncases = 0
    for it in range(220):
        nd = 1 + it % 3
        world = 1 + (it // 3) % 4
        dims = tuple(int(rng.integers(1, 14)) for _ in range(nd))
        full = np.arange(int(np.prod(dims)), dtype=np.int64).reshape(dims)
        idxs, ranks = _layout(rng, dims, world)
        sels_all = []
        for r in range(world):       # per-rank differing requests
            sels_all.append(None if rng.integers(0, 5) == 0
                            else _rand_sel(rng, dims))
        outs = _execute(full, idxs, ranks, sels_all)
        for r, sel in enumerate(sels_all):
            if sel is None:
                assert r not in outs
                continue
            res, writes = outs[r]
            assert np.all(writes == 1), (it, r, sel, idxs)
            assert np.array_equal(res, full[_ix(sel)]), (it, r, sel, idxs)
            ncases += 1
    assert ncases >= 200


def test_sel_plan_empty_chunk_and_big_step():
    full = np.arange(30, dtype=np.int64)
    idxs = [((0, 10),), ((10, 10),), ((10, 30),)]       # empty middle chunk
    ranks = [2, 0, 1]
    sel = (("a", 29, -11, 3),)                          # 29, 18, 7
    outs = _execute(full, idxs, ranks, [sel, None, sel])
    for r in (0, 2):
        assert np.array_equal(outs[r][0], full[[29, 18, 7]])
        assert np.all(outs[r][1] == 1)
    pieces = plan.sel_plan(idxs, ranks, [sel, None, sel])
    assert [(p[0], p[1]) for p in pieces] == [(1, 0), (1, 2), (2, 0), (2, 2)]
    # affine stays affine on both sides
    assert all(p[2][0][0] == "a" and p[3][0][0] == "a" for p in pieces)


def test_sel_plan_is_deterministic():
    rng = np.random.default_rng(5)
    dims = (9, 11)
    idxs, ranks = _layout(rng, dims, 4)
    sels = [_rand_sel(rng, dims) for _ in range(4)]
    a = plan.sel_plan(idxs, ranks, sels)
    b = plan.sel_plan(list(idxs), list(ranks), list(sels))
    assert len(a) == len(b)
    for p, q in zip(a, b):
        assert p[:2] == q[:2]
        for e, f in zip(p[2] + p[3], q[2] + q[3]):
            assert np.array_equal(plan.sel_indices(e), plan.sel_indices(f))
