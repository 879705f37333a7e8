"""Entity resolution over libmuninn_hip.so: the middle stages of the reference's muninn_extract_er (src/llama_er.c) —
Jaro-Winkler (src/string_sim.c), candidate pairs from neighbour lists, the scoring cascade — and the three of them behind one
call on an index's device.  Nothing here computes: every function lands in a HIP kernel (no CPU fallback).

Names are byte strings (``bytes``, or ``str`` encoded as UTF-8): the reference compares bytes, not code points.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .hnsw import ER_SYMBOLS, ErEdge, ErStats, MuninnHipError, _err, lib  # noqa: F401  (ER_SYMBOLS: bound by hnsw.lib())

GUARD = {None: 0, "": 0, "none": 0, "same_source": 1, "diff_type": 2}  # mn_er_guard; src/llama_er.c:130-136
BLOCKING = {"graph": 0, "exact": 1}  # mn_er_blocking
MAX_NAME = 4096

EDGE_DTYPE = np.dtype([("r1", np.int32), ("r2", np.int32), ("weight", np.float64)])  # mn_er_edge
assert EDGE_DTYPE.itemsize == C.sizeof(ErEdge)


def pack_names(names):
    """(bytes uint8[total], off int64[n + 1]): the arena the C-ABI takes."""
    raw = [n.encode("utf-8") if isinstance(n, str) else bytes(n) for n in names]
    off = np.zeros(len(raw) + 1, np.int64)
    if raw:
        off[1:] = np.cumsum([len(r) for r in raw])
    arena = np.frombuffer(b"".join(raw), np.uint8).copy() if off[-1] else np.zeros(0, np.uint8)
    return arena, off


def source_ids(sources):
    """int32 per entity for the type guard: 0 for an empty (or None) source, else one number per distinct value."""
    table = {}
    out = np.zeros(len(sources), np.int32)
    for i, s in enumerate(sources):
        if s is None or len(s) == 0:
            continue
        out[i] = table.setdefault(s, len(table) + 1)
    return out


def _guard(g):
    if isinstance(g, int):
        return g
    if g not in GUARD:  # the reference ignores a mode it does not know (src/llama_er.c:135-136)
        return 0
    return GUARD[g]


def jaro_winkler_packed(arena, off, a, b, device=0):
    a = np.ascontiguousarray(a, np.int32)
    b = np.ascontiguousarray(b, np.int32)
    out = np.empty(len(a), np.float64)
    if lib().mn_er_jaro_winkler(len(a), arena, off, len(off) - 1, a, b, device, out) != 0:
        raise MuninnHipError(_err())
    return out


def jaro_winkler(a, b, device=0):
    """jaro_winkler(a[p], b[p]) of src/string_sim.c:11-96 for every p, f64 bits of the reference; a, b: sequences of names."""
    if len(a) != len(b):
        raise ValueError("jaro_winkler: a and b differ in length")
    arena, off = pack_names(list(a) + list(b))
    n = len(a)
    return jaro_winkler_packed(arena, off, np.arange(n, dtype=np.int32), np.arange(n, 2 * n, dtype=np.int32), device)


def candidates(ent_ids, nbr_ids, nbr_dists, counts, dist_threshold, device=0):
    """(r1, r2, dist): the candidate pairs of src/llama_er.c:237-284 from a search's answer (ids [n][kk], f32 distances [n][kk],
    counts [n]; ent_ids [n] the entities' rowids), in the reference's order, each with its smallest distance as f64."""
    ent_ids = np.ascontiguousarray(ent_ids, np.int64).reshape(-1)
    n = len(ent_ids)
    nbr_ids = np.ascontiguousarray(nbr_ids, np.int64)
    if nbr_ids.ndim != 2 or nbr_ids.shape[0] != n:
        raise ValueError("candidates: nbr_ids must be [n][kk]")
    kk = nbr_ids.shape[1]
    nbr_dists = np.ascontiguousarray(nbr_dists, np.float32).reshape(n, kk)
    counts = np.ascontiguousarray(counts, np.int32).reshape(n)
    r1 = np.empty(max(1, n * kk), np.int32)
    r2 = np.empty(max(1, n * kk), np.int32)
    d = np.empty(max(1, n * kk), np.float64)
    m = lib().mn_er_candidates(n, kk, ent_ids, nbr_ids, nbr_dists, counts, float(dist_threshold), device, r1, r2, d)
    if m < 0:
        raise MuninnHipError(_err())
    return r1[:m].copy(), r2[:m].copy(), d[:m].copy()


def score_packed(r1, r2, dist, arena, off, source_id, guard, jw_weight, match_threshold, device=0):
    r1 = np.ascontiguousarray(r1, np.int32)
    r2 = np.ascontiguousarray(r2, np.int32)
    dist = np.ascontiguousarray(dist, np.float64)
    src = None if source_id is None else np.ascontiguousarray(source_id, np.int32)
    edges = np.empty(max(1, len(r1)), EDGE_DTYPE)
    m = lib().mn_er_score(len(r1), r1, r2, dist, len(off) - 1, arena, off, None if src is None else src.ctypes.data, _guard(guard),
                          float(jw_weight), float(match_threshold), device, edges.ctypes.data)
    if m < 0:
        raise MuninnHipError(_err())
    return edges[:m].copy()


def score(r1, r2, dist, names, sources=None, type_guard=None, jw_weight=0.5, match_threshold=0.0, device=0):
    """The type guard and scoring cascade of src/llama_er.c:295-332: a structured array (r1, r2, weight) of the candidates whose
    score reaches match_threshold, in candidate order.  sources: one value per entity (None / empty never blocks)."""
    arena, off = pack_names(names)
    return score_packed(r1, r2, dist, arena, off, None if sources is None else source_ids(sources), type_guard, jw_weight,
                        match_threshold, device)


def resolve(index, ids, names, sources=None, k=10, dist_threshold=0.15, jw_weight=0.3, borderline_delta=0.0, type_guard=None,
            blocking="graph", return_stats=False):
    """Stages 2 and 3 of muninn_extract_er on the index's device: blocking (the reference's graph search at k + 1, or
    blocking="exact": the exact k nearest under the threshold), candidate pairs, scoring cascade.  ids: the entities' rowids in
    the index (an id the index does not hold, or a deleted one, has no neighbours).  match_threshold = 1 - dist_threshold +
    borderline_delta, as the reference derives it.  Returns the match edges (r1, r2, weight), r1 < r2 indices into ids."""
    ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
    if len(names) != len(ids):
        raise ValueError("resolve: one name per id")
    arena, off = pack_names(names)
    src = None if sources is None else source_ids(sources)
    kk = k + 1 if blocking == "graph" else k
    edges = np.empty(max(1, len(ids) * max(kk, 1)), EDGE_DTYPE)
    st = ErStats()
    match_threshold = 1.0 - float(dist_threshold) + float(borderline_delta)  # src/llama_er.c:143
    m = lib().mn_hnsw_er_edges(index.h, len(ids), ids, arena, off, None if src is None else src.ctypes.data, k, float(dist_threshold),
                               float(jw_weight), match_threshold, _guard(type_guard), BLOCKING[blocking], edges.ctypes.data,
                               C.byref(st))
    if m < 0:
        raise MuninnHipError(_err())
    out = edges[:m].copy()
    if return_stats:
        return out, {name: getattr(st, name) for name, _ in ErStats._fields_}
    return out
