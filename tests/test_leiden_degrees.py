"""k_leiden_eval (csrc/mn_leiden.hip, over csrc/mn_leiden_eval.hpp) picks its code per node by the node's degree (out + in), per graph by the largest and the
mean degree, and per sweep by the sweep number.  The switches, as the source has them:

  degree <= LEI_SG_CAP (64)      a sub-group of 16 / 32 lanes evaluates the node; above: one wavefront per "wide" node (biglist)
  degree <= lds_cap              wide node staged in LDS; above (only past LEI_CAP = 1024 edges): best_move<false> in global
                                 scratch, the node's own bigoff region.  lds_cap = min(1024, max(64, round16(round4(maxdeg + 4))))
  big_log2h = 8, 9, 10           smallest table with 2^big_log2h >= lds_cap: the wide nodes' LDS layout; an unweighted wide node
                                 uses 2^lg entries of it, lg = the smallest value >= 8 with 2^lg >= its degree
  wave LDS * wpb > 60 KB         4, 2 or 1 wavefronts per workgroup (only the weighted layout ever leaves 4)
  mean degree > 48               k_leiden_eval<32, .> instead of <16, .> (one more reduction step: lei_peer<4>)
  weighted or not                best_move_wslots (list-order f64 sums, sorted operations) against best_move_hash (counts)
  synchronous sweep <= 3         sub-group table of 128 entries, 64 afterwards (for up to 64 edges)
  LEI_SYNC_CAP, LEI_GROW         hand-over from synchronous sweeps to rounds; rounds LEI_GROW times larger at the tail

Every graph below places nodes at stated degrees on both sides of these switches and at them.  The table test (CPU) restates
the arithmetic, checks that the graphs hold the degrees they claim and that together they reach every row, and runs the oracle
on each.  The device tests compare communities, the bits of Q and (moves, move sweeps, refine sweeps) with the oracle's
restatement of the same schedule: no tolerance anywhere.

Families: (A) a degree ladder in one graph, (B) a ladder of largest degrees = LDS layouts, (C) regular graphs, where gains tie
exactly, (D) multi-edges and self-loops at the boundaries, (E) tuning knobs, (F) one handle through many calls."""
import functools
import os
import re

import numpy as np
import pytest

from oracle import orc_graph as og

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = [os.path.join(ROOT, "sqlite-muninn_amd", "csrc", f) for f in ("mn_leiden_eval.hpp", "mn_leiden.hip")]  # read as one text

# the constants this table was written for (parsed out of the source and compared in the table test)
CONSTANTS = {"LEI_SG_CAP": 64, "LEI_CAP": 1024, "LEI_WPB": 4, "LEI_SYNC_CAP": 48, "LEI_PICKLESS": 3, "LEI_GROW": 4,
             "LEI_GROW_DIV": 256}
SG_CAP, CAP, WPB = 64, 1024, 4

# (A) degrees of the special nodes; each comes as all out-edges, all in-edges and a 37 / 63 split
LADDER = [0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024,
          1025, 1300]
VARIANTS = ("out", "in", "split")
# (B) largest degree of the graph -> (lds_cap, big_log2h, wavefronts per workgroup weighted).  64: no wide node (lds_cap is 80 all
# the same: it is sized from the degree + 4); 76|77 and 92|93: lds_cap 80|96|112; 252|253 and 508|509: big_log2h 8|9|10; 492|493:
# weighted wpb 4|2; 1004|1005: 2|1; 1005 and 1024: lds_cap 1024 with a node below it and a node that fills it to the last entry;
# 1025: the first node in global scratch
TOPS = {64: (80, 8, 4), 65: (80, 8, 4), 76: (80, 8, 4), 77: (96, 8, 4), 80: (96, 8, 4), 81: (96, 8, 4), 92: (96, 8, 4),
        93: (112, 8, 4), 252: (256, 8, 4), 253: (272, 9, 4), 256: (272, 9, 4), 257: (272, 9, 4), 492: (496, 9, 4),
        493: (512, 9, 2), 508: (512, 9, 2), 509: (528, 10, 2), 600: (608, 10, 2), 1004: (1008, 10, 2), 1005: (1024, 10, 1),
        1024: (1024, 10, 1), 1025: (1024, 10, 1)}
TOP_SPECIALS = (1, 17, 64)


# ───────────────────────── the dispatch arithmetic, restated ─────────────────────────

def lds_cap(maxdeg):
    max_deg = (maxdeg + 7) & ~3  # leiden_impl: int4-aligned scratch stride
    return min(CAP, max(64, (max_deg + 15) & ~15))


def big_log2h(cap):
    lg = 8
    while (1 << lg) < cap:
        lg += 1
    return lg


def node_lg(deg):
    lg = 8
    while (1 << lg) < deg:
        lg += 1
    return lg


def wave_lds(sg, hashed, cap, blg, sg_log2h=7):
    """lei_eval_lds: bytes of one wavefront (sub-group areas or one wide node's area, whichever is larger)"""
    ng = 64 // sg
    wslots = lambda c, lg: 20 * c + 10 * (1 << lg) + 16  # noqa: E731
    small = ng * (3 * (1 << sg_log2h) + 4 + SG_CAP // 2) * 4 if hashed else ng * wslots(SG_CAP, 6)
    big = 3 * (1 << blg) * 4 + 16 + ((cap * 2 + 15) & ~15) if hashed else wslots(cap, blg)
    return (max(small, big) + 15) & ~15


def wpb(wlds):
    w = WPB
    while w > 1 and wlds * w > 60 * 1024:
        w >>= 1
    return w


def sub_group(n, n_edges):
    return 32 if 2.0 * n_edges / max(1, n) > 48.0 else 16


def degrees(n, s, d):
    return np.bincount(s, minlength=n) + np.bincount(d, minlength=n)


# ───────────────────────── graph generators ─────────────────────────

def _background(n, blocks, m, r):
    """n nodes in `blocks` planted blocks (block = index % blocks), m edges, 85 % of them inside a block"""
    s = r.integers(0, n, m)
    d_in = (s % blocks) + blocks * r.integers(0, n // blocks, m)
    d = np.where(r.random(m) < 0.85, d_in, r.integers(0, n, m))
    keep = s != d
    return s[keep], d[keep]


def _weights(kind, m, r):
    if kind == "u":
        return None
    if kind == "q":
        return r.integers(1, 9, m) * 0.25  # quarters: many equal sums
    if kind == "h":
        return np.full(m, 0.5)
    return r.random(m) * 3 + 0.01


def _attach(nb, specials, positions, bg_s, bg_d, r, shuffle=True):
    """Special node i = (degree, variant) sits at node index positions[i]; its edges go to DISTINCT background nodes (so every
    neighbour carries a label of its own in the first sweep: tables are full at the powers of two).  Background node b gets
    the b-th index not taken by a special node."""
    n = nb + len(specials)
    free = np.setdiff1d(np.arange(n), np.asarray(positions))
    ss, dd = [free[bg_s]], [free[bg_d]]
    for (deg, var), pos in zip(specials, positions):
        t = free[r.choice(nb, deg, replace=False)]
        n_out = {"out": deg, "in": 0, "split": int(round(0.37 * deg))}[var]
        me = np.full(deg, pos)
        ss += [me[:n_out], t[n_out:]]
        dd += [t[:n_out], me[n_out:]]
    s, d = np.concatenate(ss), np.concatenate(dd)
    if shuffle:
        o = r.permutation(len(s))
        s, d = s[o], d[o]
    return n, s.astype(np.int32), d.astype(np.int32)


@functools.lru_cache(maxsize=None)
def ladder():
    """(A) 2 600 background nodes in 20 blocks + 93 special nodes, spread over the first 830 indices so that rounds of 64 and of
    512 hold several wide nodes and several scratch nodes each; wide nodes sit on both sides of the round edges 63|64 and
    511|512 (big0 / big1 slice biglist there).  → n, src, dst, {index: (degree, variant)}"""
    r = np.random.default_rng(20240)
    specials = [(deg, var) for deg in LADDER for var in VARIANTS]
    specials = [specials[i] for i in r.permutation(len(specials))]
    positions = list(range(1, 1 + 9 * len(specials), 9))
    positions[6], positions[56], positions[57] = 63, 511, 512  # (positions[7] is 64)
    for slot, want in ((6, (1300, "out")), (7, (65, "in")), (56, (1025, "split")), (57, (1024, "out"))):
        j = specials.index(want)
        specials[slot], specials[j] = specials[j], specials[slot]
    bs, bd = _background(2600, 20, 7000, r)
    n, s, d = _attach(2600, specials, positions, bs, bd, r)
    return n, s, d, dict(zip(positions, specials))


@functools.lru_cache(maxsize=None)
def top_graph(top):
    """(B) 1 200 background nodes in 12 blocks + nodes of degree 1, 17, 64 and `top` (37 / 63 split), `top` the largest degree"""
    r = np.random.default_rng(7000 + top)
    specials = [(deg, "split") for deg in TOP_SPECIALS + (top,)]
    positions = [5, 300, 301, 700]
    bs, bd = _background(1200, 12, 3600, r)
    n, s, d = _attach(1200, specials, positions, bs, bd, r)
    return n, s, d, dict(zip(positions, specials))


def circulant(n, k):
    i = np.repeat(np.arange(n), k)
    j = np.tile(np.arange(1, k + 1), n)
    return n, i.astype(np.int32), ((i + j) % n).astype(np.int32)


def complete(n):
    i, j = np.triu_indices(n, 1)
    return n, i.astype(np.int32), j.astype(np.int32)


def bipartite(a, b):
    i = np.repeat(np.arange(a), b)
    j = a + np.tile(np.arange(b), a)
    return a + b, i.astype(np.int32), j.astype(np.int32)


CHUNK_HUBS = {0: (200, (70, 130, 131)), 1: (1100, (64, 128, 700, 1030))}  # hub index: (degree, list positions of the tying leaves)


@functools.lru_cache(maxsize=None)
def chunk_tie():
    """(C) best_move walks a list in chunks of 64 edges and lets a later chunk replace the best one only on a strictly larger
    gain.  Two hubs (out-edges only, edge order kept): at the stated list positions a hub points at a leaf (degree 1), everywhere
    else at a member of a K_6 of its own.  Against singletons the gain of joining t is w/m - res k_v k_t / 2m², so the leaves
    tie exactly at the top and first show up in chunks 1, 2, (10, 16).  Hub 1 has more than 1 024 edges (best_move<false> in the
    parallel schedules), hub 0 fewer (best_move in the sequential kernel; the position rule of the table kernels otherwise)."""
    s, d = [], []
    nxt = len(CHUNK_HUBS)
    for hub, (deg, ties) in CHUNK_HUBS.items():
        members = []
        for _ in range((deg + 5) // 6):
            q = list(range(nxt, nxt + 6))
            nxt += 6
            members += q
            for a in range(6):
                for b in range(a + 1, 6):
                    s.append(q[a])
                    d.append(q[b])
        for p in range(deg):
            if p in ties:
                t, nxt = nxt, nxt + 1
            else:
                t = members.pop()
            s.append(hub)
            d.append(t)
    return nxt, np.asarray(s, np.int32), np.asarray(d, np.int32)


MULTI = {10: 64, 11: 66, 200: 65, 201: 200}  # (D) node index: degree


@functools.lru_cache(maxsize=None)
def multi():
    """(D) on 600 background nodes: node 10 = 32 targets listed twice (degree 64), node 11 = 33 targets twice (66), node 200 =
    63 edges + a self-loop, which sits in both lists (65), node 201 = 200 edges, half of them to one neighbour"""
    r = np.random.default_rng(515)
    bs, bd = _background(600, 6, 1800, r)
    n, s, d = _attach(600, [(0, "out")] * 4, list(MULTI), bs, bd, r, shuffle=False)
    free = np.setdiff1d(np.arange(n), list(MULTI))
    t32, t33, t63, t101 = (free[r.choice(600, k, replace=False)] for k in (32, 33, 63, 101))
    es = [np.full(64, 10), np.full(66, 11), np.full(40, 200), t63[40:], [200], np.full(150, 201), np.full(50, t101[0])]
    ed = [np.tile(t32, 2), np.tile(t33, 2), t63[:40], np.full(23, 200), [200],
          np.concatenate([np.full(50, t101[0]), t101[1:]]), np.full(50, 201)]
    s, d = np.concatenate([s] + es), np.concatenate([d] + ed)
    o = r.permutation(len(s))
    return n, s[o].astype(np.int32), d[o].astype(np.int32)


def clique_hub(deg):
    """(D) node 0 points at one member each of `deg` K_4: its neighbours stay in `deg` different communities for good, so the
    table of a node with 64 edges is still (all but) full after the third sweep, when it has 64 entries"""
    s, d = [], []
    for c in range(deg):
        q = [1 + 4 * c + i for i in range(4)]
        s += [0] + [q[a] for a in range(4) for b in range(a + 1, 4)]
        d += [q[0]] + [q[b] for a in range(4) for b in range(a + 1, 4)]
    return 1 + 4 * deg, np.asarray(s, np.int32), np.asarray(d, np.int32)


def _case(family, build, kinds, claims):
    return {f"{family}_{k}": (build, k, claims) for k in kinds}


# name -> (builder of (n, src, dst, ...), weight kind, degrees the case claims to contain)
CASES = {}
CASES.update(_case("ladder", ladder, "uqr", tuple(LADDER)))
for _t in TOPS:
    CASES.update(_case(f"top{_t}", functools.partial(top_graph, _t), "ur", TOP_SPECIALS + (_t,)))
REGULAR = {"circ400_32": (functools.partial(circulant, 400, 32), (64,)), "circ400_33": (functools.partial(circulant, 400, 33), (66,)),
           "circ120_24": (functools.partial(circulant, 120, 24), (48,)), "circ120_25": (functools.partial(circulant, 120, 25), (50,)),
           "k65": (functools.partial(complete, 65), (64,)), "k66": (functools.partial(complete, 66), (65,)),
           "k40_90": (functools.partial(bipartite, 40, 90), (40, 90)), "chunk_tie": (chunk_tie, (1, 200, 1100))}
for _n, (_b, _c) in REGULAR.items():
    CASES.update(_case(_n, _b, "uh", _c))
CASES.update(_case("multi", multi, "ur", tuple(MULTI.values())))
CASES.update(_case("cliquehub64", functools.partial(clique_hub, 64), "uh", (64,)))
CASES.update(_case("cliquehub65", functools.partial(clique_hub, 65), "uh", (65,)))
LADDERS = ["ladder_u", "ladder_q", "ladder_r"]
TOP_CASES = [f"top{t}_{k}" for t in TOPS for k in "ur"]
REGULAR_CASES = [f"{n}_{k}" for n in REGULAR for k in "uh"]
MULTI_CASES = ["multi_u", "multi_r", "cliquehub64_u", "cliquehub64_h", "cliquehub65_u", "cliquehub65_h"]


@functools.lru_cache(maxsize=None)
def graph(name):
    """→ (n, src, dst, w): the weights are drawn per case from a seed of their own, after the edges"""
    build, kind, _ = CASES[name]
    n, s, d = build()[:3]
    return n, s, d, _weights(kind, len(s), np.random.default_rng(len(s) + ord(kind)))


@functools.lru_cache(maxsize=None)
def csr(name):
    n, s, d, w = graph(name)
    return og.Csr(s, d, w, "both", n_nodes=n, first_seen=False)


_REF = {}


def reference(name, res, batch, env=()):
    """orc_leiden on the case, computed once per (case, resolution, schedule, oracle settings) and shared"""
    key = (name, res, batch, tuple(env))
    if key not in _REF:
        saved = {k: os.environ.get(k) for k, _ in env}
        try:
            for k, v in env:
                os.environ[k] = v
            comm, q, st = og.leiden(csr(name), res, batch)
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        comm.setflags(write=False)
        _REF[key] = (comm, q, st)
    return _REF[key]


def qbits(q):
    return np.array([q], np.float64).view(np.int64)[0]


# ───────────────────────── 0. the table, on the CPU ─────────────────────────

def test_source_constants_are_the_ones_the_table_was_written_for():
    text = "\n".join(open(p).read() for p in SRCS)
    for name, want in CONSTANTS.items():
        found = re.findall(rf"^#define\s+{name}\s+(\d+)\b", text, re.M)
        assert found == [str(want)], (name, found)
    assert (SG_CAP, CAP, WPB) == (CONSTANTS["LEI_SG_CAP"], CONSTANTS["LEI_CAP"], CONSTANTS["LEI_WPB"])


def test_every_graph_holds_the_degrees_its_case_claims():
    for name, (_, _, claims) in CASES.items():
        n, s, d, w = graph(name)
        assert n < 3000 and len(s) < 30000, name
        assert (w is None) == name.endswith("_u"), name
        deg = degrees(n, s, d)
        assert set(claims) <= set(deg.tolist()), (name, sorted(set(claims) - set(deg.tolist())))
    # (A) the special nodes have exactly their degree in each of the three variants, nothing else is wide, their neighbours
    # are distinct background nodes, and a round of 64 / 512 holds several wide / several scratch nodes
    n, s, d, special = ladder()
    deg, out = degrees(n, s, d), np.bincount(s, minlength=n)
    assert sorted(special.values()) == sorted((g, v) for g in LADDER for v in VARIANTS)
    for pos, (g, var) in special.items():
        assert deg[pos] == g and out[pos] == {"out": g, "in": 0, "split": int(round(0.37 * g))}[var], (pos, g, var)
        nb = np.concatenate([d[s == pos], s[d == pos]])
        assert len(set(nb.tolist())) == g and not set(nb.tolist()) & set(special), pos
    assert any(0 < out[p] < g and out[p] % 4 for p, (g, v) in special.items() if v == "split" and g > SG_CAP)
    wide = np.nonzero(deg > SG_CAP)[0]
    assert set(wide.tolist()) == {p for p, (g, _) in special.items() if g > SG_CAP}
    assert all(deg[p] > SG_CAP for p in (63, 64, 511, 512))  # wide nodes on both sides of a round edge of 64 and of 512
    scratch = np.nonzero(deg > CAP)[0]
    assert len(scratch) == 6 and np.bincount(wide // 64).max() >= 3
    assert np.bincount(scratch // 512).max() >= 2 and np.bincount(scratch // 64).max() >= 2
    assert sub_group(n, len(s)) == 16
    # (B) the largest degree is `top`, held by one node; lds_cap, big_log2h and the weighted wpb are what the table states
    for top, (cap, blg, w_wpb) in TOPS.items():
        n, s, d, special = top_graph(top)
        deg = degrees(n, s, d)
        assert deg.max() == top and [deg[p] for p in special] == list(TOP_SPECIALS + (top,)), top
        assert (lds_cap(top), big_log2h(lds_cap(top))) == (cap, blg), top
        assert wpb(wave_lds(16, False, cap, blg)) == w_wpb and wpb(wave_lds(16, True, cap, blg)) == 4, top
        assert (np.count_nonzero(deg > SG_CAP) == 0) == (top == 64), top
    # (C), (D)
    for name, (build, claims) in REGULAR.items():
        n, s, d = build()
        if name != "chunk_tie":
            assert set(degrees(n, s, d).tolist()) == set(claims), name
    n, s, d = chunk_tie()
    deg = degrees(n, s, d)
    for hub, (g, ties) in CHUNK_HUBS.items():
        lst = d[s == hub]  # out-edges only, in edge order = list order
        assert deg[hub] == g == len(lst) and len(set(lst.tolist())) == g
        assert [p for p in range(g) if deg[lst[p]] == 1] == list(ties) and all(deg[lst[p]] == 6 for p in range(g) if p not in ties)
        assert {p // 64 for p in ties} >= {1, 2} and 0 not in {p // 64 for p in ties}
    n, s, d = multi()
    deg = degrees(n, s, d)
    assert {v: int(deg[v]) for v in MULTI} == MULTI
    assert len(set(d[s == 10].tolist())) == 32 and len(set(d[s == 11].tolist())) == 33
    assert np.count_nonzero((s == 200) & (d == 200)) == 1 and deg[200] - 2 == 63
    nb201 = np.concatenate([d[s == 201], s[d == 201]])
    assert np.bincount(nb201).max() == 100
    for g in (64, 65):
        n, s, d = clique_hub(g)
        assert degrees(n, s, d)[0] == g and degrees(n, s, d)[1:].max() == 4


def test_cases_reach_every_row_of_the_dispatch_table():
    deg_of = {name: degrees(*graph(name)[:3]) for name in CASES}
    both = lambda names: {n[-1] != "u" for n in names} == {True, False}  # noqa: E731
    with_deg = lambda g: [n for n in CASES if (deg_of[n] == g).any()]  # noqa: E731
    # sub-group | wide node, weighted and not: at the switch, one past it, and well on either side
    for g in (1, 63, SG_CAP, SG_CAP + 1, SG_CAP + 2, 129):
        assert both(with_deg(g)), g
    # LDS | global scratch: a node that fills lds_cap = LEI_CAP to the last entry, one past it, one far past it
    assert lds_cap(CAP) == CAP == lds_cap(1300) and big_log2h(CAP) == 10
    for g in (CAP - 1, CAP, CAP + 1, 1300):
        assert both(with_deg(g)), g
    # an unweighted wide node's table, 2^lg entries: full to the last entry (degree 2^lg), one edge past it (next size), one short
    for lg in (8, 9, 10):
        assert node_lg(1 << lg) == lg and both(with_deg(1 << lg)) and both(with_deg((1 << lg) - 1))
        if lg < 10:
            assert node_lg((1 << lg) + 1) == lg + 1 and both(with_deg((1 << lg) + 1))
    assert node_lg(SG_CAP + 1) == 8 and node_lg(1 << 7) == 8  # (no wide table below 256 entries)
    # lds_cap steps by 16, big_log2h by one and the weighted wpb halves between neighbouring entries of TOPS, on both sides
    tops = sorted(TOPS)
    caps = {t: lds_cap(t) for t in range(SG_CAP, CAP + 2)}
    for lo, hi in ((76, 77), (92, 93)):
        assert lo in TOPS and hi in TOPS and caps[hi] == caps[lo] + 16
    for lo, hi in ((252, 253), (508, 509)):
        assert lo in TOPS and hi in TOPS and big_log2h(caps[hi]) == big_log2h(caps[lo]) + 1
    w_wpb = {t: wpb(wave_lds(16, False, caps[t], big_log2h(caps[t]))) for t in caps}
    assert [t for t in caps if t > SG_CAP and w_wpb[t] != w_wpb[t - 1]] == [493, 1005]  # every place where it changes ...
    assert {492, 493, 1004, 1005} <= set(TOPS) and {w_wpb[t] for t in tops} == {4, 2, 1}  # ... has a case on each side
    assert {wpb(wave_lds(sg, True, caps[t], big_log2h(caps[t]), lg)) for t in caps for sg in (16, 32) for lg in (6, 7)} == {4}
    assert {big_log2h(caps[t]) for t in tops} == {8, 9, 10} and caps[64] == caps[65] == 80
    # the comment on LeiArgs::big_log2h: the table holds one entry per edge, 2^big_log2h >= lds_cap is all the code provides
    assert all((1 << big_log2h(c)) >= c for c in caps.values()) and any((1 << big_log2h(c)) < 2 * c for c in caps.values())
    # mean degree > 48: 32 lanes per node; 48.0 exactly is still 16
    sg = {name: sub_group(graph(name)[0], len(graph(name)[1])) for name in CASES}
    assert sg["circ120_24_u"] == 16 and sg["circ120_25_u"] == 32 and sg["circ120_25_h"] == 32
    assert deg_of["circ120_25_u"].max() <= SG_CAP  # <32, .> with every node in a sub-group
    assert sg["circ400_32_u"] == 32 and sg["circ400_33_h"] == 32 and deg_of["circ400_33_u"].min() > SG_CAP  # <32, .>, all wide
    assert sg["k65_u"] == 32 and sg["k66_h"] == 32 and sg["k40_90_u"] == 32 and sg["ladder_u"] == 16 and sg["top1025_r"] == 16


def test_schedule_switches_are_reached(capfd, monkeypatch):
    """sweep <= 3 | later, a synchronous phase that settles | is handed over to rounds at the cap, and the tail rule on and off,
    read from the oracle's trace"""
    monkeypatch.setenv("ORC_LEIDEN_TRACE", "1")
    og.leiden(csr("top1025_r"), 1.0, -3)
    err = capfd.readouterr().err
    assert "sync sweep 3 (pick-less)" in err and "sync sweep 4:" in err and "rounds of" not in err  # settles within the cap
    og.leiden(csr("ladder_q"), 1.0, -3)
    err = capfd.readouterr().err
    assert "sync sweep 48 (pick-less)" in err and "sync sweep 49" not in err  # LEI_SYNC_CAP, then lei_round_default(2 693) = 256
    assert "rounds of 256:" in err and "rounds of 1024:" in err
    monkeypatch.setenv("ORC_LEI_SYNC_CAP", "2")
    og.leiden(csr("top1025_r"), 1.0, -3)
    err = capfd.readouterr().err
    assert "sync sweep 2:" in err and "sync sweep 3" not in err and "rounds of 256:" in err
    monkeypatch.delenv("ORC_LEI_SYNC_CAP")
    og.leiden(csr("ladder_q"), 1.0, 64)
    err = capfd.readouterr().err
    assert "rounds of 64:" in err and "rounds of 256:" in err  # LEI_GROW = 4 times larger at the tail
    monkeypatch.setenv("ORC_LEI_GROW", "16,8")
    og.leiden(csr("ladder_q"), 1.0, 64)
    assert "rounds of 1024:" in capfd.readouterr().err
    monkeypatch.setenv("ORC_LEI_GROW", "1,256")
    og.leiden(csr("ladder_q"), 1.0, 64)
    err = capfd.readouterr().err
    assert "rounds of 64:" in err and "rounds of 256:" not in err


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_terminates_with_contiguous_ids(name):
    for batch in (1, 64, -3):
        comm, q, st = reference(name, 1.0, batch)
        assert sorted(set(comm.tolist())) == list(range(int(comm.max()) + 1)), (name, batch)
        assert st["moves"] > 0 and st["move_sweeps"] > 0 and np.isfinite(q), (name, batch)
        if name.startswith(("k65", "k66")):
            assert comm.max() == 0 and q == 0.0, (name, batch)  # K_n: one community
    if name.startswith("cliquehub"):  # the hub's neighbours end in different communities: its table stays full
        comm = reference(name, 1.0, -3)[0]
        n, s, d, _ = graph(name)
        assert len(set(comm[d[s == 0]].tolist())) == len(d[s == 0]) and reference(name, 1.0, -3)[2]["move_sweeps"] > 3


# ───────────────────────── the device against the oracle ─────────────────────────

SEQ, R64, R512, SYNC, SYNC2 = "sequential", 64, 512, 0, -2


class Dev:
    """one device handle of a case"""

    def __init__(self, gpu, name):
        c = csr(name)
        self.gpu, self.name = gpu, name
        self.g = gpu.Graph(c.n, c.off_out, c.tgt_out, c.w_out if c.weighted else None, c.off_in, c.tgt_in,
                           c.w_in if c.weighted else None)

    def check(self, mode, res=1.0, env=(), orc_batch=None):
        """mode: SEQ, a round size, SYNC (the default schedule: device batch 0 = the oracle's -3) or a negative period"""
        if orc_batch is None:
            orc_batch = 1 if mode == SEQ else -3 if mode == SYNC else mode
        oc, oq, ost = reference(self.name, res, orc_batch, env)
        if mode == SEQ:
            comm, q, st = self.g.leiden(res, "both", self.gpu.LEIDEN_SEQUENTIAL)
        else:
            comm, q, st = self.g.leiden(res, "both", self.gpu.LEIDEN_BATCHED, mode)
        what = (self.name, mode, res, env)
        print(what, "moves/sweeps device", (st["moves"], st["move_sweeps"], st["refine_sweeps"]), "oracle",
              (ost["moves"], ost["move_sweeps"], ost["refine_sweeps"]), "Q", q, oq, "differing nodes", int((comm != oc).sum()))
        assert np.array_equal(comm, oc), what
        assert qbits(q) == qbits(oq), what
        assert (st["moves"], st["move_sweeps"], st["refine_sweeps"]) == (ost["moves"], ost["move_sweeps"], ost["refine_sweeps"]), what

    def close(self):
        self.g.close()


@pytest.fixture
def dev(gpu):
    made = []

    def make(name):
        made.append(Dev(gpu, name))
        return made[-1]

    yield make
    for x in made:
        x.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode,res", [(SEQ, 1.0), (R64, 1.0), (R64, 0.3), (R512, 1.0), (R512, 1.7), (SYNC, 1.0), (SYNC, 0.3),
                                      (SYNC2, 1.0), (SYNC2, 1.7)])
@pytest.mark.parametrize("name", LADDERS)
def test_degree_ladder(dev, name, mode, res):
    """(A) every degree of LADDER in one graph: sub-group nodes, wide nodes with tables of 256, 512 and 1 024 entries full to the
    last one, and the global-scratch nodes, several of each per round"""
    dev(name).check(mode, res)


@pytest.mark.gpu
@pytest.mark.parametrize("name", TOP_CASES)
def test_largest_degree_ladder(dev, name):
    """(B) one LDS layout per largest degree (lds_cap, big_log2h, wavefronts per workgroup): synchronous sweeps and rounds"""
    x = dev(name)
    x.check(SYNC)
    x.check(R64)
    x.check(R512, 1.7)


@pytest.mark.gpu
@pytest.mark.parametrize("name", REGULAR_CASES)
def test_regular_graphs_where_gains_tie(dev, name):
    """(C) every lane of a reduction holds the same gain: the first-position rule decides, across lanes (lei_best_step) and
    across 64-edge chunks (best_move).  circ120_25: k_leiden_eval<32, .> with every node in a sub-group."""
    x = dev(name)
    x.check(SEQ)
    x.check(R64)
    x.check(SYNC)


@pytest.mark.gpu
@pytest.mark.parametrize("name", MULTI_CASES)
def test_multi_edges_and_self_loops_at_the_boundaries(dev, name):
    """(D) repeated targets, a self-loop that makes a node wide, a node with half its edges to one neighbour; and hubs whose
    neighbours never merge"""
    x = dev(name)
    x.check(SEQ)
    x.check(R64)
    x.check(SYNC)
    x.check(SYNC2, 1.7)


KNOB_CASES = ["ladder_u", "ladder_q", "circ120_25_u", "circ120_25_h"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", KNOB_CASES)
@pytest.mark.parametrize("sg", ["16", "32"])
def test_sub_group_width_is_speed_only(dev, monkeypatch, name, sg):
    """(E) MN_LEIDEN_SG: both widths on both graphs (the ladder's default is 16, the circulant's 32)"""
    monkeypatch.setenv("MN_LEIDEN_SG", sg)
    x = dev(name)
    x.check(SYNC)
    x.check(R64)


@pytest.mark.gpu
@pytest.mark.parametrize("name", KNOB_CASES)
def test_full_tables_is_speed_only(dev, monkeypatch, name):
    monkeypatch.setenv("MN_LEIDEN_FULL_TABLES", "1")
    dev(name).check(SYNC)


@pytest.mark.gpu
@pytest.mark.parametrize("name", KNOB_CASES)
@pytest.mark.parametrize("cap", ["0", "2", "5"])
def test_sync_cap_hands_over_to_rounds_on_both_sides_alike(dev, monkeypatch, name, cap):
    monkeypatch.setenv("MN_LEIDEN_SYNC_CAP", cap)
    dev(name).check(SYNC, env=(("ORC_LEI_SYNC_CAP", cap),))


@pytest.mark.gpu
@pytest.mark.parametrize("name", KNOB_CASES)
@pytest.mark.parametrize("grow", ["16,8", "1,256"])
def test_tail_rule_settings_on_both_sides_alike(dev, monkeypatch, name, grow):
    """16,8: the workspace is sized for rounds 16 times larger; 1,256: the tail rule is off"""
    monkeypatch.setenv("MN_LEIDEN_GROW", grow)
    dev(name).check(R64, env=(("ORC_LEI_GROW", grow),))


@pytest.mark.gpu
@pytest.mark.parametrize("name", KNOB_CASES)
def test_batch_knob_selects_rounds(dev, monkeypatch, name):
    monkeypatch.setenv("MN_LEIDEN_BATCH", "300")
    dev(name).check(SYNC, orc_batch=300)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ladder_r", "ladder_u"])
def test_one_handle_many_calls(dev, monkeypatch, name):
    """(F) LeiWork is kept per graph and grown on demand (batch_cap, ocap, scratch_have, the big_mode cache): each call of a
    sequence that grows it step by step equals its oracle answer"""
    x = dev(name)
    x.check(R64)
    x.check(R512)
    x.check(SYNC)
    x.check(SEQ)
    monkeypatch.setenv("MN_LEIDEN_GROW", "16,8")
    x.check(R64, env=(("ORC_LEI_GROW", "16,8"),))
    monkeypatch.delenv("MN_LEIDEN_GROW")
    x.check(SYNC)
