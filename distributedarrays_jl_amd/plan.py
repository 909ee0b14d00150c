"""Communication plans for the distributed matmul — pure data, no GPU.

Re-expresses the reference's _matmatmul! dataflow
(/root/reference/src/linalg.jl:190-253) over xGMI point-to-point:

  reference                              MI355X-native
  ---------                              -------------
  caller slices B[Acuts2[j], Ccuts[k]]   b-slab all-to-all: each rank
  (DArray getindex => remote gather,     (i,j) receives the B row-slab
   linalg.jl:215)                        Acuts2[j] x (all cols) from B's
                                         owners via grouped ncclSend/Recv
  R[i,j,k] = remotecall owner(A[i,j])    local MFMA GEMM on the slab panel
  (linalg.jl:218-226)
  C-owner fetches R[i,j,k], add!         partial-exchange: rank (i,j)
  (linalg.jl:243-251)                    sends partial k to C-owner (i,k);
                                         owner adds in ascending j

Plans are deterministic sorted lists so every rank derives the identical
send/recv schedule (RCCL grouped calls must pair up).  Tested on CPU
(tests/test_plan.py, tests/test_gloo.py) against the oracle.
"""
import numpy as np

from . import geometry
from ._ffi import DArrayError


def c_grid(A_dist, B_dist):
    """C's process grid: procs(A)[:, 1:q], q = min(J, B cols-chunks)
    (linalg.jl:266-272)."""
    I, J = A_dist
    K = min(J, B_dist[1] if len(B_dist) > 1 else 1)
    return (I, K)


def a_rank_pos(r, A_dist):
    """Rank r's (i, j) in A's column-major grid; None if r holds no A."""
    I, J = A_dist
    if r >= I * J:
        return None
    return (r % I, r // I)


def slab_rows(A_cuts2, j):
    """Rows of B needed by A-column j: Acuts[j]:Acuts[j+1]-1
    (linalg.jl:213-215)."""
    return geometry.ranges1d(A_cuts2)[j]


def bslab_plan(A_dist, A_cuts2, B_dims, B_dist, B_idxs):
    """All-to-all pieces (src, dst, rows, cols) in GLOBAL coordinates:
    rank dst=(i,j) needs B rows slab_rows(j) x all cols; owner src holds
    block B_idxs[src].  Sorted deterministically."""
    I, J = A_dist
    nB = 1
    for c in B_dist:
        nB *= c
    pieces = []
    for dst in range(I * J):
        i, j = dst % I, dst // I
        rneed = slab_rows(A_cuts2, j)
        for src in range(nB):
            rows_s, cols_s = B_idxs[src][0], B_idxs[src][1]
            inter = geometry.intersect1d(rneed, rows_s)
            if inter is not None and cols_s[1] > cols_s[0]:
                pieces.append((src, dst, inter, cols_s))
    pieces.sort()
    return pieces


def partial_plan(A_dist, K):
    """(src, dst, k) triples: rank (i,j) ships its k-th partial product
    to C-owner (i,k) = rank i + I*k (linalg.jl:243-251); j==k stays
    local.  Sorted deterministically."""
    I, J = A_dist
    moves = []
    for r in range(I * J):
        i, j = r % I, r // I
        for k in range(K):
            owner = i + I * k
            if owner != r:
                moves.append((r, owner, k))
    moves.sort()
    return moves


def halo_plan(src_idxs, src_ranks, boxes):
    """Pieces (src_rank, dst_rank, box) for the makelocal halo gather
    (darray.jl:351-368: requested indices not fully local are fetched
    from the owning chunks; here via grouped ncclSend/Recv).

    src_idxs: chunk boxes of the source DArray; src_ranks[c] = owner.
    boxes[r]: the box rank r requests (None = no request).  Returns a
    deterministic sorted list in GLOBAL coordinates."""
    pieces = []
    for dst, box in enumerate(boxes):
        if box is None:
            continue
        for c, idx in enumerate(src_idxs):
            inter = []
            ok = True
            for (blo, bhi), (clo, chi) in zip(box, idx):
                lo, hi = max(blo, clo), min(bhi, chi)
                if hi <= lo:
                    ok = False
                    break
                inter.append((lo, hi))
            if ok:
                pieces.append((src_ranks[c], dst, tuple(inter)))
    pieces.sort()
    return pieces


def accumulate_order(J):
    """Owner-side add! order over j (ascending — one valid schedule of
    the reference's async accumulation, linalg.jl:243-251)."""
    return list(range(J))


# ------------------------------------------------- strided / vector indexing
# A *selection* is a tuple with one entry per dimension of the indexed
# array: ("a", start, step, count) selects start + j*step for 0 <= j <
# count (step may be negative; 0 only with count <= 1), ("v", int64 array)
# selects the listed indices in order (unsorted and repeated entries are
# fine on the read side).  All indices are 0-based.  Several subscripts
# combine as an OUTER PRODUCT, as in Julia (M[[0,2],[1,3]] is
# m[np.ix_([0,2],[1,3])]), not numpy's zipped fancy indexing.

def is_int(k):
    return isinstance(k, (int, np.integer)) and not isinstance(k, (bool, np.bool_))


def sel_normalize(subs, dims):
    """Subscript tuple -> (selection, squeeze).  Accepts ints, slices
    (any step, resolved by slice.indices(dim), so ::-1 and 5::-2 work),
    ranges, and integer lists / 1-D integer arrays with every entry in
    [0, dim).  Ints become one-element affine entries and their
    dimensions are listed in `squeeze` (dropped from the result shape,
    as Julia drops scalar-indexed dimensions)."""
    if not isinstance(subs, tuple):
        subs = (subs,)
    if len(subs) != len(dims):
        raise DArrayError("indexing needs %d subscripts" % len(dims))
    sel, squeeze = [], []
    for d, (k, dim) in enumerate(zip(subs, dims)):
        if is_int(k):
            k = int(k)
            if not 0 <= k < dim:
                raise DArrayError("index %d outside [0, %d) in dimension %d"
                                  % (k, dim, d))
            sel.append(("a", k, 1, 1))
            squeeze.append(d)
        elif isinstance(k, (slice, range)):
            r = range(*k.indices(dim)) if isinstance(k, slice) else k
            n = len(r)
            if n and not (0 <= r[0] < dim and 0 <= r[-1] < dim):
                raise DArrayError("range %r outside [0, %d) in dimension %d"
                                  % (k, dim, d))
            sel.append(("a", int(r.start), int(r.step), n) if n
                       else ("a", 0, 1, 0))
        elif isinstance(k, (list, tuple, np.ndarray)):
            v = np.asarray(k)
            if v.size == 0:
                v = v.astype(np.int64)
            if v.ndim != 1 or v.dtype.kind not in "iu":
                raise DArrayError(
                    "index vector in dimension %d must be a 1-D integer "
                    "list or array (boolean masks are not supported)" % d)
            v = np.ascontiguousarray(v, dtype=np.int64)
            if v.size and (v.min() < 0 or v.max() >= dim):
                raise DArrayError("index vector entry outside [0, %d) in "
                                  "dimension %d" % (dim, d))
            sel.append(("v", v))
        else:
            raise DArrayError("bad subscript %r" % (k,))
    return tuple(sel), tuple(squeeze)


def sel_full(dims):
    """The selection of a whole array."""
    return tuple(("a", 0, 1, int(n)) for n in dims)


def sel_from_box(box):
    """Half-open per-dimension ranges -> selection."""
    return tuple(("a", int(lo), 1, int(hi - lo)) for lo, hi in box)


def sel_count(e):
    return int(e[3]) if e[0] == "a" else int(e[1].size)


def sel_shape(sel):
    return tuple(sel_count(e) for e in sel)


def sel_indices(e):
    """The selected indices of one dimension as an int64 array."""
    if e[0] == "a":
        return e[1] + e[2] * np.arange(e[3], dtype=np.int64)
    return e[1]


def sel_has_duplicates(sel):
    """True when a selection names some element twice (a repeated vector
    entry; affine entries with count > 1 always have a non-zero step)."""
    for e in sel:
        if e[0] == "v" and np.unique(e[1]).size != e[1].size:
            return True
        if e[0] == "a" and e[3] > 1 and e[2] == 0:
            return True
    return False


def _compose1(o, i):
    if o[0] == "a":
        if i[0] == "a":
            return ("a", o[1] + i[1] * o[2], o[2] * i[2], i[3]) if i[3] \
                else ("a", 0, 1, 0)
        return ("v", o[1] + o[2] * i[1])
    return ("v", np.ascontiguousarray(o[1][sel_indices(i)]))


def compose(outer, inner):
    """Selection of a selection: `inner` indexes the array that `outer`
    selects (so inner's entries lie in [0, count of outer)); the result
    selects the same elements straight from outer's parent."""
    if len(outer) != len(inner):
        raise DArrayError("compose: %d vs %d dimensions"
                          % (len(outer), len(inner)))
    for d, (o, i) in enumerate(zip(outer, inner)):
        n = sel_count(o)
        ix = sel_indices(i)
        if ix.size and (ix.min() < 0 or ix.max() >= n):
            raise DArrayError("compose: dimension %d index outside [0, %d)"
                              % (d, n))
    return tuple(_compose1(o, i) for o, i in zip(outer, inner))


def sel_expand(sel, ndims, squeeze):
    """A selection written in a squeezed index space -> all `ndims`
    dimensions, with a one-element entry at every squeezed one."""
    it = iter(sel)
    out = tuple(("a", 0, 1, 1) if d in squeeze else next(it)
                for d in range(ndims))
    if next(it, None) is not None:
        raise DArrayError("indexing needs %d subscripts"
                          % (ndims - len(squeeze)))
    return out


def _cdiv(a, b):
    return -((-a) // b)


def _intersect1(e, lo, hi):
    """One dimension of a selection against the chunk interval [lo, hi):
    (local_entry, position_entry) or None when nothing falls inside.  An
    affine entry meets an interval in a contiguous stretch of positions,
    so both results stay affine."""
    if hi <= lo:
        return None
    if e[0] == "a":
        _, s, st, n = e
        if n == 0:
            return None
        if st > 0:
            j0, j1 = max(0, _cdiv(lo - s, st)), min(n - 1, (hi - 1 - s) // st)
        elif st < 0:
            j0, j1 = max(0, _cdiv(s - (hi - 1), -st)), min(n - 1,
                                                           (s - lo) // -st)
        else:
            j0, j1 = (0, n - 1) if lo <= s < hi else (1, 0)
        if j1 < j0:
            return None
        m = j1 - j0 + 1
        return ("a", s + j0 * st - lo, st, m), ("a", j0, 1, m)
    v = e[1]
    pos = np.nonzero((v >= lo) & (v < hi))[0].astype(np.int64)
    if pos.size == 0:
        return None
    loc = ("v", np.ascontiguousarray(v[pos] - lo))
    if pos[-1] - pos[0] == pos.size - 1:
        return loc, ("a", int(pos[0]), 1, int(pos.size))
    return loc, ("v", pos)


def sel_intersect(sel, idx):
    """A selection against one chunk box: (local_sel, pos_sel) — the
    chunk-local indices of the selected elements that the chunk holds, and
    their positions in the selection's result — or None if there are
    none."""
    loc, pos = [], []
    for e, (lo, hi) in zip(sel, idx):
        r = _intersect1(e, lo, hi)
        if r is None:
            return None
        loc.append(r[0])
        pos.append(r[1])
    return tuple(loc), tuple(pos)


def sel_plan(src_idxs, src_ranks, sels_all):
    """Pieces (src_rank, dst_rank, src_local_sel, dst_pos_sel) of the
    selection gather, the strided analogue of halo_plan: sels_all[r] is
    the selection rank r requests in the source's GLOBAL index space (or
    None); each piece is what one source chunk contributes, as
    chunk-local indices on the source side and positions in r's packed
    result on the destination side.  Empty pieces are dropped.  The list
    is sorted by (src_rank, dst_rank, chunk) from metadata every rank
    shares, so sends and receives pair up in FIFO order."""
    keyed = []
    for dst, sel in enumerate(sels_all):
        if sel is None:
            continue
        for c, idx in enumerate(src_idxs):
            r = sel_intersect(sel, idx)
            if r is not None:
                keyed.append(((src_ranks[c], dst, c),
                              (src_ranks[c], dst, r[0], r[1])))
    keyed.sort(key=lambda kp: kp[0])
    return [p for _, p in keyed]
