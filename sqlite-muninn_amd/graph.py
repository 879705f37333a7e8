"""Host-side mirror of the reference's graph hot path over libmuninn_hip.so: device-resident CSR
adjacency (src/graph_csr.h) and run_leiden (src/graph_community.c:336).  ctypes only; no compute here."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .hnsw import MuninnHipError, lib

LEIDEN_SEQUENTIAL, LEIDEN_BATCHED = 0, 1

_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")


class LeidenStats(C.Structure):
    _fields_ = [("iterations", C.c_int64), ("moves", C.c_int64), ("move_sweeps", C.c_int64), ("refine_sweeps", C.c_int64),
                ("n_communities", C.c_int), ("device_ms", C.c_double)]


class BfsStats(C.Structure):
    _fields_ = [("rows", C.c_int64), ("levels", C.c_int64), ("chunks", C.c_int64), ("edges_scanned", C.c_int64),
                ("device_ms", C.c_double)]


class DfsStats(C.Structure):
    _fields_ = [("rows", C.c_int64), ("chunks", C.c_int64), ("entries_scanned", C.c_int64), ("max_frames", C.c_int64),
                ("device_ms", C.c_double)]


class SpStats(C.Structure):
    _fields_ = [("mode_used", C.c_int), ("chunks", C.c_int), ("sources", C.c_int), ("pops", C.c_int64), ("pushes", C.c_int64),
                ("relaxations", C.c_int64), ("passes", C.c_int64), ("device_ms", C.c_double)]


SP_AUTO, SP_REPLAY, SP_FAST, SP_UNWEIGHTED = range(4)
SP_MODES = {"auto": SP_AUTO, "replay": SP_REPLAY, "exact": SP_REPLAY, "fast": SP_FAST}


class SelectOp(C.Structure):
    _fields_ = [("op", C.c_int), ("node", C.c_int), ("depth_up", C.c_int), ("depth_down", C.c_int), ("name_off", C.c_int),
                ("name_len", C.c_int)]


class SelectStats(C.Structure):
    _fields_ = [("rows", C.c_int64), ("levels", C.c_int64), ("launches", C.c_int64), ("syncs", C.c_int64),
                ("bottom_up_levels", C.c_int64), ("device_ms", C.c_double)]


SEL_NODE, SEL_ANCESTORS, SEL_DESCENDANTS, SEL_BOTH, SEL_CLOSURE, SEL_UNION, SEL_INTERSECT, SEL_COMPLEMENT = range(8)
SELECT_LEVELS_PER_SYNC = 16  # the library's default for MN_SELECT_LEVELS_PER_SYNC (csrc/mn_select.hip)
SEL_DIRECTIONS = ("self", "ancestor", "descendant", "both", "closure", "selected", "selected", "selected")


class N2vParams(C.Structure):
    _fields_ = [("dim", C.c_int), ("p", C.c_double), ("q", C.c_double), ("num_walks", C.c_int), ("walk_length", C.c_int),
                ("window", C.c_int), ("neg_samples", C.c_int), ("learning_rate", C.c_double), ("epochs", C.c_int),
                ("batch_walks", C.c_int)]


class N2vStats(C.Structure):
    _fields_ = [("pairs", C.c_int64), ("device_ms", C.c_double)]


N2V_SEQUENTIAL, N2V_BATCHED = 0, 1
COMPONENTS_EXACT, COMPONENTS_FAST = 0, 1


class AlgoStats(C.Structure):
    _fields_ = [("device_ms", C.c_double), ("iterations", C.c_int), ("aux", C.c_int64)]


GRAPH_SYMBOLS = [
    ("mn_node2vec_train", C.c_int, [C.c_int, _i32p, _i32p, C.POINTER(N2vParams), C.c_int, C.c_int,
                                    np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"), C.POINTER(N2vStats)]),
    ("mn_node2vec_last_error", C.c_char_p, []),
    ("mn_node2vec_train_shared", C.c_int, [C.c_void_p, C.c_int, _i32p, _i32p, C.POINTER(N2vParams), C.c_int,
                                           np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"), C.POINTER(N2vStats)]),
    ("mn_n2v_begin", C.c_void_p, [C.c_int, _i32p, _i32p, C.POINTER(N2vParams), C.c_int]),
    ("mn_n2v_batch_walks", C.c_int, [C.c_void_p]),
    ("mn_n2v_sample_slots", C.c_int, [C.c_void_p]),
    ("mn_n2v_position_slots", C.c_int, [C.c_void_p]),
    ("mn_n2v_samples", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p]),
    ("mn_n2v_apply", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]),
    ("mn_n2v_sync", C.c_int, [C.c_void_p]),
    ("mn_n2v_finish", C.c_int, [C.c_void_p, np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"), C.POINTER(N2vStats)]),
    ("mn_n2v_finish_dev", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(N2vStats)]),
    ("mn_node2vec_train_into", C.c_int, [C.c_int, _i32p, _i32p, C.POINTER(N2vParams), C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                         C.POINTER(N2vStats), C.POINTER(C.c_double)]),
    ("mn_n2v_end", None, [C.c_void_p]),
    ("mn_graph_create", C.c_void_p, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    ("mn_graph_create_blocked", C.c_void_p, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]),
    ("mn_graph_from_edges", C.c_void_p, [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    ("mn_graph_export_csr", C.c_int, [C.c_void_p, C.c_int, _i32p, C.c_void_p, C.c_void_p]),
    ("mn_graph_retain", None, [C.c_void_p]),
    ("mn_graph_destroy", None, [C.c_void_p]),
    ("mn_graph_last_error", C.c_char_p, []),
    ("mn_graph_leiden", C.c_int, [C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_int, _i32p, C.POINTER(C.c_double)]),
    ("mn_graph_leiden_stats", C.c_int, [C.c_void_p, C.POINTER(LeidenStats)]),
    ("mn_graph_leiden_shared", C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_int, _i32p, C.POINTER(C.c_double)]),
    ("mn_graph_betweenness", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS"),
                                       C.c_void_p]),
    ("mn_graph_last_ms", C.c_double, [C.c_void_p]),
    ("mn_graph_out_edge_count", C.c_longlong, [C.c_void_p]),
    ("mn_graph_out_lists", C.c_int, [C.c_void_p, _i32p, _i32p]),
    ("mn_graph_closeness", C.c_int, [C.c_void_p, C.c_int, C.c_int, np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")]),
    ("mn_graph_degree", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("mn_graph_bfs", C.c_int64, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int,
                                 np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS"), C.POINTER(BfsStats)]),
    ("mn_graph_bfs_rows", C.c_int, [C.c_void_p, _i32p, _i32p, _i32p]),
    ("mn_graph_dfs", C.c_int64, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int,
                                 np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS"), C.POINTER(DfsStats)]),
    ("mn_graph_dfs_rows", C.c_int, [C.c_void_p, _i32p, _i32p, _i32p]),
    ("mn_graph_shortest_paths", C.c_int64, [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                            np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS"), C.POINTER(SpStats)]),
    ("mn_graph_shortest_paths_rows", C.c_int, [C.c_void_p, _i32p, np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")]),
    ("mn_select_parse", C.c_int, [C.c_char_p, C.POINTER(C.POINTER(SelectOp)), C.POINTER(C.c_int)]),
    ("mn_graph_select", C.c_int64, [C.c_void_p, C.POINTER(SelectOp), C.c_int, C.POINTER(SelectStats)]),
    ("mn_graph_select_rows", C.c_int, [C.c_void_p, _i32p, _i32p]),
    ("mn_graph_pagerank", C.c_int, [C.c_int, C.c_int64, _i32p, _i32p, C.c_double, C.c_int, C.c_int,
                                    np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS"), C.POINTER(AlgoStats)]),
    ("mn_graph_components", C.c_int, [C.c_int, C.c_int64, _i32p, _i32p, C.c_int, C.c_int, _i32p, _i32p, C.POINTER(AlgoStats)]),
    ("mn_graph_algo_last_error", C.c_char_p, []),
    ("mn_csr_apply_delta", C.c_int, [C.c_int, _i32p, _i32p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, _i32p,
                                     C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    ("mn_host_free", None, [C.c_void_p]),
]


def _glib():
    L = lib()
    if not getattr(L, "_graph_bound", False):
        for name, res, args in GRAPH_SYMBOLS:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        L._graph_bound = True
    return L


def _gerr():
    m = _glib().mn_graph_last_error()
    return m.decode() if m else ""


class CsrBlock(C.Structure):
    _fields_ = [("offsets", C.c_void_p), ("offsets_bytes", C.c_int), ("targets", C.c_void_p), ("targets_bytes", C.c_int),
                ("weights", C.c_void_p), ("weights_bytes", C.c_int)]


class Graph:
    """Device copy of GraphData.out / GraphData.in as CSR.  off/tgt int32, weights float64 or None."""

    def __init__(self, n, off_out, tgt_out, w_out, off_in, tgt_in, w_in, device=0):
        self.L = _glib()
        self.n = int(n)
        keep = [np.ascontiguousarray(off_out, np.int32), np.ascontiguousarray(tgt_out, np.int32),
                None if w_out is None else np.ascontiguousarray(w_out, np.float64),
                np.ascontiguousarray(off_in, np.int32), np.ascontiguousarray(tgt_in, np.int32),
                None if w_in is None else np.ascontiguousarray(w_in, np.float64)]
        ptr = lambda a: None if a is None else a.ctypes.data
        self.h = self.L.mn_graph_create(self.n, ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), ptr(keep[4]), ptr(keep[5]),
                                        device)
        if not self.h:
            raise MuninnHipError("mn_graph_create failed: " + _gerr())

    @classmethod
    def from_blocks(cls, n, fwd, rev, device=0):
        """fwd / rev: lists of (offsets bytes, targets bytes, weights bytes | None) — the rows of the reference's
        "{t}_csr_fwd" / "{t}_csr_rev" shadow tables in block_id order (mn_graph_create_blocked)."""
        self = cls.__new__(cls)
        self.L = _glib()
        self.n = int(n)

        def pack(rows):
            arr = (CsrBlock * max(1, len(rows)))()
            keep = []
            for i, (o, t, w) in enumerate(rows):
                bufs = [C.create_string_buffer(bytes(x), len(x)) if x else None for x in (o, t, w)]
                keep.append(bufs)
                arr[i] = CsrBlock(C.cast(bufs[0], C.c_void_p) if bufs[0] else None, len(o) if o else 0,
                                  C.cast(bufs[1], C.c_void_p) if bufs[1] else None, len(t) if t else 0,
                                  C.cast(bufs[2], C.c_void_p) if bufs[2] else None, len(w) if w else 0)
            return arr, keep

        fa, k1 = pack(fwd)
        ra, k2 = pack(rev)
        self.h = self.L.mn_graph_create_blocked(self.n, C.byref(fa), len(fwd), C.byref(ra), len(rev), device)
        if not self.h:
            raise MuninnHipError("mn_graph_create_blocked failed: " + _gerr())
        return self

    @classmethod
    def from_edges(cls, n, src, dst, weights=None, lists="both", device=0):
        """The graph of an edge list with integer node indices, built on the device (mn_graph_from_edges): out[src] lists
        dst and in[dst] lists src in row order, as csr_pair_from_edges gives them.  lists: "out", "in" or "both"."""
        self = cls.__new__(cls)
        self.L = _glib()
        self.n = int(n)
        s, d = np.ascontiguousarray(src, np.int32).reshape(-1), np.ascontiguousarray(dst, np.int32).reshape(-1)
        if len(s) != len(d):
            raise ValueError("from_edges: src and dst differ in length")
        w = None if weights is None else np.ascontiguousarray(weights, np.float64).reshape(-1)
        if w is not None and len(w) != len(s):
            raise ValueError("from_edges: weights and rows differ in length")
        self.h = self.L.mn_graph_from_edges(self.n, len(s), s.ctypes.data, d.ctypes.data, None if w is None else w.ctypes.data,
                                            {"out": 1, "in": 2, "both": 3}[lists], device)
        if not self.h:
            raise MuninnHipError("mn_graph_from_edges failed: " + _gerr())
        return self

    def export_csr(self, which="out"):
        """One direction as the host's CSR (mn_graph_export_csr) → (off int32[n + 1], tgt int32[E], w float64[E] or None);
        which: "out" / 0 or "in" / 1.  w is None where the graph holds no weights for that direction."""
        k = {"out": 0, "in": 1, 0: 0, 1: 1}[which]
        off = np.zeros(self.n + 1, np.int32)
        if self.L.mn_graph_export_csr(self.h, k, off, None, None) < 0:
            raise MuninnHipError(_gerr())
        e = int(off[-1])
        tgt, w = np.zeros(e, np.int32), np.zeros(e, np.float64)
        rc = self.L.mn_graph_export_csr(self.h, k, off, tgt.ctypes.data, w.ctypes.data)
        if rc < 0:
            raise MuninnHipError(_gerr())
        return off, tgt, (w if rc == 1 else None)

    def close(self):
        if getattr(self, "h", None):
            self.L.mn_graph_destroy(self.h)
            self.h = None

    __del__ = close

    def betweenness(self, direction="forward", auto_approx=0, normalized=0, edges=False):
        """brandes_compute (src/graph_centrality.c:393-505) → (cb[n], eb[n][n] or None, device ms)"""
        cb = np.zeros(max(self.n, 1), np.float64)
        eb = np.zeros((self.n, self.n), np.float64) if edges else None
        d = {"both": 0, "forward": 1, "reverse": 2}[direction]
        if self.L.mn_graph_betweenness(self.h, d, int(auto_approx), int(normalized), cb, eb.ctypes.data if edges else None) != 0:
            raise MuninnHipError(_gerr())
        return cb[:self.n], eb, self.L.mn_graph_last_ms(self.h)

    def closeness(self, direction="forward", normalized=1):
        """clo_filter's per-source loop (src/graph_centrality.c:1396-1434) → (cc[n], device ms)"""
        cc = np.zeros(max(self.n, 1), np.float64)
        d = {"both": 0, "forward": 1, "reverse": 2}[direction]
        if self.L.mn_graph_closeness(self.h, d, int(normalized), cc) != 0:
            raise MuninnHipError(_gerr())
        return cc[:self.n], self.L.mn_graph_last_ms(self.h)

    def degree(self, normalized=0):
        """deg_filter's loop (src/graph_centrality.c:667-680) → (in_degree[n], out_degree[n], degree[n], centrality[n])"""
        out = [np.zeros(max(self.n, 1), np.float64) for _ in range(4)]
        if self.L.mn_graph_degree(self.h, int(normalized), *[a.ctypes.data for a in out]) != 0:
            raise MuninnHipError(_gerr())
        return tuple(a[:self.n] for a in out)

    def bfs_batch(self, seeds, max_depth=100, direction="forward"):
        """run_bfs (src/graph_tvf.c:230-309) from every seed at once → (row_off[len(seeds) + 1] int64, node, depth, parent
        int32): seed i's rows, in the reference's queue order, are row_off[i] .. row_off[i + 1] - 1; parent is -1 for a
        seed's own row.  The call's statistics are in self.bfs_stats afterwards."""
        seeds = np.ascontiguousarray(seeds, np.int32).reshape(-1)
        row_off = np.zeros(len(seeds) + 1, np.int64)
        st = BfsStats()
        d = {"both": 0, "forward": 1, "reverse": 2}[direction]
        rows = self.L.mn_graph_bfs(self.h, d, len(seeds), seeds.ctypes.data if len(seeds) else None, int(max_depth), row_off,
                                   C.byref(st))
        if rows < 0:
            raise MuninnHipError(_gerr())
        out = [np.empty(max(rows, 1), np.int32) for _ in range(3)]
        if self.L.mn_graph_bfs_rows(self.h, *out) != 0:
            raise MuninnHipError(_gerr())
        self.bfs_stats = {n: getattr(st, n) for n, _ in BfsStats._fields_}
        return (row_off,) + tuple(a[:rows] for a in out)

    def bfs(self, seed, max_depth=100, direction="forward"):
        """graph_bfs's rows from one start node → (node, depth, parent) int32 arrays; self.bfs_stats as for bfs_batch"""
        return self.bfs_batch([seed], max_depth, direction)[1:]

    def dfs_batch(self, seeds, max_depth=100, direction="forward"):
        """run_dfs (src/graph_tvf.c:322-416) from every seed at once → (row_off[len(seeds) + 1] int64, node, depth, parent
        int32): seed i's rows, in the reference's pop order, are row_off[i] .. row_off[i + 1] - 1; parent is -1 for a seed's
        own row.  One wavefront per seed (csrc/mn_dfs.hip).  The call's statistics are in self.dfs_stats afterwards."""
        seeds = np.ascontiguousarray(seeds, np.int32).reshape(-1)
        row_off = np.zeros(len(seeds) + 1, np.int64)
        st = DfsStats()
        d = {"both": 0, "forward": 1, "reverse": 2}[direction]
        rows = self.L.mn_graph_dfs(self.h, d, len(seeds), seeds.ctypes.data if len(seeds) else None, int(max_depth), row_off,
                                   C.byref(st))
        if rows < 0:
            raise MuninnHipError(_gerr())
        out = [np.empty(max(rows, 1), np.int32) for _ in range(3)]
        if self.L.mn_graph_dfs_rows(self.h, *out) != 0:
            raise MuninnHipError(_gerr())
        self.dfs_stats = {n: getattr(st, n) for n, _ in DfsStats._fields_}
        return (row_off,) + tuple(a[:rows] for a in out)

    def dfs(self, seed, max_depth=100, direction="forward"):
        """graph_dfs's rows from one start node → (node, depth, parent) int32 arrays; self.dfs_stats as for dfs_batch"""
        return self.dfs_batch([seed], max_depth, direction)[1:]

    def select_program(self, prog):
        """selector_eval (src/graph_selector_eval.c:511-543) for a resolved program, a list of (op, node, depth_up,
        depth_down) → (node, depth) int32 arrays in ascending node index; self.select_stats afterwards"""
        ops = (SelectOp * max(1, len(prog)))()
        for i, (op, node, up, down) in enumerate(prog):
            ops[i] = SelectOp(int(op), int(node), int(up), int(down), 0, 0)
        st = SelectStats()
        rows = self.L.mn_graph_select(self.h, ops, len(prog), C.byref(st))
        if rows < 0:
            raise MuninnHipError(_gerr())
        out = [np.empty(max(rows, 1), np.int32) for _ in range(2)]
        if self.L.mn_graph_select_rows(self.h, *out) != 0:
            raise MuninnHipError(_gerr())
        self.select_stats = {n: getattr(st, n) for n, _ in SelectStats._fields_}
        return tuple(a[:rows] for a in out)

    def select(self, expr, names=None):
        """graph_select's rows for a selector expression → (node int32, depth int32, direction str).  names: the node ids by
        index, as the edge table gave them, or a function from a name's bytes to its index (-1: no such node); None → a
        node's name is its index in decimal.  ValueError carries the reference's message: a syntax error, or the first
        name, left to right, that is no node."""
        prog = select_parse(expr)
        if self.n == 0:  # selector_eval answers an empty graph before it looks anything up (:514)
            return np.zeros(0, np.int32), np.zeros(0, np.int32), SEL_DIRECTIONS[prog[-1][0]]
        index = None if names is None or callable(names) else {}
        for i, nm in enumerate(() if index is None else names):
            index.setdefault(nm.encode() if isinstance(nm, str) else bytes(nm), i)
        resolved = []
        for op, name, up, down in prog:
            node = -1
            if op <= SEL_CLOSURE:
                if index is not None:
                    node = index.get(name, -1)
                elif callable(names):
                    node = int(names(name))
                    node = node if 0 <= node < self.n else -1
                elif name.isdigit() and name == b"%d" % int(name) and int(name) < self.n:
                    node = int(name)
                if node < 0:
                    msg = b"graph_select: node '" + name + b"' not found"
                    raise ValueError(msg[:255].decode("utf-8", "replace"))  # snprintf into 256 bytes (:287)
            resolved.append((op, node, up, down))
        node, depth = self.select_program(resolved)
        return node, depth, SEL_DIRECTIONS[prog[-1][0]]

    def shortest_paths(self, starts, ends, weighted=True, mode="auto"):
        """graph_shortest_path's search (src/graph_tvf.c:472-753) for the pairs (starts[i], ends[i]) at once → (row_off
        [len(starts) + 1] int64, node int32, distance float64): pair i's path, start first, is rows row_off[i] ..
        row_off[i + 1] - 1 (none when end is not reached).  mode "replay" (or "exact") gives the reference's rows, "fast" its
        distances and the canonical path, "auto" chooses (include/muninn_hip.h); weighted=False, or a graph without weights,
        is the reference's BFS half.  The call's statistics are in self.sp_stats afterwards."""
        starts = np.ascontiguousarray(starts, np.int32).reshape(-1)
        ends = np.ascontiguousarray(ends, np.int32).reshape(-1)
        if len(starts) != len(ends):
            raise ValueError("shortest_paths: starts and ends differ in length")
        row_off = np.zeros(len(starts) + 1, np.int64)
        st = SpStats()
        rows = self.L.mn_graph_shortest_paths(self.h, SP_MODES[mode], int(bool(weighted)), len(starts),
                                              starts.ctypes.data if len(starts) else None, ends.ctypes.data if len(ends) else None,
                                              row_off, C.byref(st))
        if rows < 0:
            raise MuninnHipError(_gerr())
        node, dist = np.empty(max(rows, 1), np.int32), np.empty(max(rows, 1), np.float64)
        if self.L.mn_graph_shortest_paths_rows(self.h, node, dist) != 0:
            raise MuninnHipError(_gerr())
        self.sp_stats = {n: getattr(st, n) for n, _ in SpStats._fields_}
        return row_off, node[:rows], dist[:rows]

    def shortest_path(self, start, end, weighted=True, mode="auto"):
        """one pair of shortest_paths → (node int32, distance float64), empty when end is not reached"""
        return self.shortest_paths([start], [end], weighted, mode)[1:]

    def shortest_path_unweighted(self, start, end):
        """run_shortest_path_bfs (src/graph_tvf.c:472-586): the first-discovery parents of a forward BFS from start, traced
        back from end → the nodes of the path, start first, or [] when end is not reached."""
        return [int(v) for v in self.shortest_path(start, end, weighted=False)[0]]

    def leiden(self, resolution=1.0, direction="both", mode=LEIDEN_SEQUENTIAL, batch=0):
        """run_leiden → (community[n] int32, Q, stats dict)"""
        comm = np.empty(max(self.n, 1), np.int32)
        q = C.c_double(0.0)
        rc = self.L.mn_graph_leiden(self.h, float(resolution), 1 if direction == "both" else 0, mode, batch, comm, C.byref(q))
        if rc != 0:
            raise MuninnHipError(_gerr())
        st = LeidenStats()
        self.L.mn_graph_leiden_stats(self.h, C.byref(st))
        return comm[:self.n], q.value, {n: getattr(st, n) for n, _ in LeidenStats._fields_}


def select_parse(expr):
    """selector_parse (src/graph_selector_parse.c) → the postfix program as a list of (op, name bytes or None, depth_up,
    depth_down), atoms in source order.  ValueError carries the reference's message.  Touches no device."""
    L = _glib()
    raw = expr.encode("utf-8", "surrogateescape") if isinstance(expr, str) else bytes(expr)
    raw = raw.split(b"\0", 1)[0]  # a C string ends at its first NUL
    prog, n = C.POINTER(SelectOp)(), C.c_int(0)
    if L.mn_select_parse(raw, C.byref(prog), C.byref(n)) != 0:
        raise ValueError((L.mn_graph_last_error() or b"").decode("utf-8", "surrogateescape"))
    try:
        return [(o.op, raw[o.name_off:o.name_off + o.name_len] if o.op <= SEL_CLOSURE else None, o.depth_up, o.depth_down)
                for o in (prog[i] for i in range(n.value))]
    finally:
        L.mn_host_free(prog)


def node2vec_train(off, adj, dim, p=1.0, q=1.0, num_walks=10, walk_length=80, window=5, neg_samples=5, learning_rate=0.025,
                   epochs=1, mode=N2V_SEQUENTIAL, device=0, batch_walks=0):
    """node2vec_train's compute (src/node2vec.c:486-551) on the device → (embeddings [n][dim] f32, stats)."""
    L = _glib()
    off = np.ascontiguousarray(off, np.int32)
    adj = np.ascontiguousarray(adj if len(adj) else np.zeros(1, np.int32), np.int32)
    n = len(off) - 1
    out = np.zeros((max(n, 1), dim), np.float32)
    prm = N2vParams(dim, p, q, num_walks, walk_length, window, neg_samples, learning_rate, epochs, batch_walks)
    st = N2vStats()
    rc = L.mn_node2vec_train(n, off, adj, C.byref(prm), mode, device, out, C.byref(st))
    if rc < 0:
        m = L.mn_node2vec_last_error()
        raise MuninnHipError(m.decode() if m else "mn_node2vec_train failed")
    return out[:n], {"pairs": st.pairs, "device_ms": st.device_ms}


# ───────────── host-side CSR builders (the device input formats; node ids are already indices) ─────────────

def csr_pair_from_edges(n, src, dst, weights=None):
    """GraphData.out / GraphData.in as CSR (src/graph_csr.c:20-70 over src/graph_load.c:218-246): out[src] lists dst
    and in[dst] lists src, each in edge order.  → (off_out, tgt_out, w_out, off_in, tgt_in, w_in); weights None ⇒ None."""
    src = np.asarray(src, np.int64)
    dst = np.asarray(dst, np.int64)
    w = None if weights is None else np.asarray(weights, np.float64)

    def one(keys, vals):
        o = np.argsort(keys, kind="stable")
        off = np.zeros(n + 1, np.int64)
        np.add.at(off, keys + 1, 1)
        return np.cumsum(off).astype(np.int32), vals[o].astype(np.int32), None if w is None else w[o].copy()

    return one(src, dst) + one(dst, src)


def graph_from_edges(n, src, dst, weights=None, device=0):
    """Graph (Leiden input) from an edge list with integer node indices."""
    return Graph(n, *csr_pair_from_edges(n, src, dst, weights), device=device)


def node2vec_train_into(off, adj, dim, index, first_rowid=1, want_embeddings=True, p=1.0, q=1.0, num_walks=10, walk_length=80,
                        window=5, neg_samples=5, learning_rate=0.025, epochs=1, batch_walks=0):
    """mn_node2vec_train_into: train (MN_N2V_BATCHED) on the index's device and build `index` (an hnsw.HnswIndex) from the
    embeddings without a host round trip → (embeddings [n][dim] f32 or None, stats with 'build_seconds')."""
    L = _glib()
    off = np.ascontiguousarray(off, np.int32)
    adj = np.ascontiguousarray(adj if len(adj) else np.zeros(1, np.int32), np.int32)
    n = len(off) - 1
    out = np.zeros((max(n, 1), dim), np.float32) if want_embeddings else None
    prm = N2vParams(dim, p, q, num_walks, walk_length, window, neg_samples, learning_rate, epochs, batch_walks)
    st = N2vStats()
    bs = C.c_double(0.0)
    rc = L.mn_node2vec_train_into(n, off, adj, C.byref(prm), N2V_BATCHED, index.h, int(first_rowid),
                                  out.ctypes.data if out is not None else None, C.byref(st), C.byref(bs))
    if rc < 0:
        raise MuninnHipError((L.mn_node2vec_last_error() or b"").decode())
    return (out[:n] if out is not None else None), {"pairs": st.pairs, "device_ms": st.device_ms, "build_seconds": bs.value}


def n2v_csr_from_edges(n, src, dst):
    """node2vec.c's own adjacency (src/node2vec.c:96-134): undirected, duplicate edges dropped, every list in
    insertion order (edge i adds src→dst, then dst→src).  → (off int32[n+1], adj int32[E])."""
    src = np.asarray(src, np.int64)
    dst = np.asarray(dst, np.int64)
    a = np.empty(2 * len(src), np.int64)
    b = np.empty(2 * len(src), np.int64)
    a[0::2], a[1::2] = src, dst
    b[0::2], b[1::2] = dst, src
    _, first = np.unique(a * n + b, return_index=True)
    first.sort()
    a, b = a[first], b[first]
    o = np.argsort(a, kind="stable")
    off = np.zeros(n + 1, np.int64)
    np.add.at(off, a + 1, 1)
    return np.cumsum(off).astype(np.int32), b[o].astype(np.int32)


# ───────────── f-4: graph_tvf.c's edge-list algorithms (nodes = first-seen indices, edges in row order) ─────────────

def _edges(src, dst):
    src, dst = np.ascontiguousarray(src, np.int32), np.ascontiguousarray(dst, np.int32)
    pad = np.zeros(1, np.int32)
    return (src if len(src) else pad), (dst if len(dst) else pad), len(src)


def pagerank(n, src, dst, damping=0.85, iterations=20, device=0):
    """run_pagerank (src/graph_tvf.c:1631-1797) → (rank[n] float64, stats)"""
    L = _glib()
    s, d, ne = _edges(src, dst)
    out = np.zeros(max(n, 1), np.float64)
    st = AlgoStats()
    if L.mn_graph_pagerank(n, ne, s, d, float(damping), int(iterations), device, out, C.byref(st)) != 0:
        raise MuninnHipError((L.mn_graph_algo_last_error() or b"").decode())
    return out[:n], {"device_ms": st.device_ms, "iterations": st.iterations, "dangling": st.aux}


def components(n, src, dst, mode=COMPONENTS_EXACT, device=0):
    """run_components (src/graph_tvf.c:1314-1366) → (component_id[n], component_size[n], stats)"""
    L = _glib()
    s, d, ne = _edges(src, dst)
    cid, csz = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    st = AlgoStats()
    if L.mn_graph_components(n, ne, s, d, mode, device, cid, csz, C.byref(st)) != 0:
        raise MuninnHipError((L.mn_graph_algo_last_error() or b"").decode())
    return cid[:n], csz[:n], {"device_ms": st.device_ms, "rounds": st.iterations}


class CsrDelta(C.Structure):  # CsrDelta, src/graph_csr.h:37-42
    _fields_ = [("src_idx", C.c_int32), ("dst_idx", C.c_int32), ("weight", C.c_double), ("op", C.c_int)]


def csr_apply_delta(off, tgt, w, dsrc, ddst, dw, dop, new_n, device=0):
    """csr_apply_delta (src/graph_csr.c:175-325) on the device → (new_off, new_tgt, new_w or None)"""
    L = _glib()
    off = np.ascontiguousarray(off, np.int32)
    old_n = len(off) - 1
    tgt = np.ascontiguousarray(tgt if len(tgt) else np.zeros(1, np.int32), np.int32)
    wv = None if w is None else np.ascontiguousarray(w if len(w) else np.zeros(1), np.float64)
    nd = len(dsrc)
    dl = (CsrDelta * max(nd, 1))()
    for i in range(nd):
        dl[i] = CsrDelta(int(dsrc[i]), int(ddst[i]), float(dw[i]), int(dop[i]))
    new_off = np.zeros(max(new_n, old_n) + 1, np.int32)
    pt, pw, ne = C.c_void_p(), C.c_void_p(), C.c_int(0)
    rc = L.mn_csr_apply_delta(old_n, off, tgt, None if wv is None else wv.ctypes.data, 0 if wv is None else 1, dl, nd, new_n, device,
                              new_off, C.byref(pt), C.byref(pw), C.byref(ne))
    if rc != 0:
        raise MuninnHipError((L.mn_graph_algo_last_error() or b"").decode())
    e = ne.value
    new_tgt = np.ctypeslib.as_array(C.cast(pt, C.POINTER(C.c_int32)), (e,)).copy() if e else np.zeros(0, np.int32)
    new_w = None
    if wv is not None:
        new_w = np.ctypeslib.as_array(C.cast(pw, C.POINTER(C.c_double)), (e,)).copy() if e else np.zeros(0, np.float64)
    L.mn_host_free(pt)
    L.mn_host_free(pw)
    return new_off, new_tgt, new_w
