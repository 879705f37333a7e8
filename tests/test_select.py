"""Graph.select on the device against tests/select_model.py (itself held to the compiled reference's recorded rows by
tests/test_select_model.py): whole rows equal — node, depth, direction — or the same error.  Every shape runs with the
bottom-up step forced off, forced on and chosen per level, and with one level per status read-back and the default group:
none of these may change a row.  The shapes are the smallest at which each kernel can go wrong: the last word of a set, list
lengths around the wavefront and workgroup widths, frontiers around a word and a workgroup, contested claims, depth limits
around the group size."""
import os
import random

import numpy as np
import pytest

import select_model as sm

MODES = [(bu, lps) for bu in ("0", "1", "auto") for lps in ("1", None)]


def name_of(i):
    return "n%d" % i


def index_of(name):
    return int(name[1:]) if name[:1] == b"n" and name[1:].isdigit() else -1


class Case:
    """a graph on the device and its answers from the model, computed once per expression"""

    def __init__(self, mn, n, src, dst):
        self.n, self.src, self.dst = n, np.asarray(src, np.int64), np.asarray(dst, np.int64)
        self.g = mn.graph.graph_from_edges(n, self.src, self.dst)
        self.lists = sm.lists_of(n, self.src, self.dst)

    def want(self, expr):
        try:
            rows, direction = sm.evaluate(sm.parse(expr), self.n, self.lists[0], self.lists[1], index_of)
            return [r[0] for r in rows], [r[1] for r in rows], direction
        except sm.SelectError as e:
            return e.args[0].decode()

    def got(self, expr):
        try:
            node, depth, direction = self.g.select(expr, names=index_of)
            return node.tolist(), depth.tolist(), direction
        except ValueError as e:
            return e.args[0]

    def check(self, exprs, modes=MODES):
        saved = {k: os.environ.pop(k, None) for k in ("MN_SELECT_BOTTOM_UP", "MN_SELECT_LEVELS_PER_SYNC", "MN_SELECT_BOTTOM_UP_DIV")}
        try:
            for expr in exprs:
                want = self.want(expr)
                for bu, lps in modes:
                    os.environ["MN_SELECT_BOTTOM_UP"] = bu
                    if lps is None:
                        os.environ.pop("MN_SELECT_LEVELS_PER_SYNC", None)
                    else:
                        os.environ["MN_SELECT_LEVELS_PER_SYNC"] = lps
                    assert self.got(expr) == want, (expr, bu, lps)
        finally:
            for k, v in saved.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v

    def close(self):
        self.g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129])
def test_last_word_of_complement_and_rows(gpu, n):
    """a path over all n nodes (n = 1: a self-loop): `not x` and `not x+` must not report a node at or above n"""
    src, dst = (np.arange(n - 1), np.arange(1, n)) if n > 1 else ([0], [0])
    c = Case(gpu, n, src, dst)
    x, last = name_of(n // 2), name_of(n - 1)
    c.check([f"not {x}", f"not {x}+", f"not {x}+1", f"not {x}+0", f"not {last}", f"not +{last}", "not n0", f"{x}+ not {x}+1", f"{x}+,+{x}",
             f"+{last}+", f"@{x}", "n0+1"])
    c.close()


HUB_LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 1025, 5000]


def hub_targets(first, d):
    """d list entries over fewer nodes than entries: duplicates among them"""
    distinct = max(1, d - d // 4)
    return [first + (j * 7) % distinct for j in range(d)], distinct


@pytest.mark.gpu
@pytest.mark.parametrize("d", HUB_LENGTHS)
def test_hub_as_the_seed(gpu, d):
    """node 0 lists d entries; every target lists one node further on; a last node lists nothing"""
    tg, distinct = hub_targets(1, d)
    n = 1 + distinct + 2
    src = [0] * d + list(range(1, 1 + distinct))
    dst = tg + [1 + distinct] * distinct
    c = Case(gpu, n, src, dst)
    far = name_of(1 + distinct)
    c.check(["n0+", "n0+1", "n0+2", f"+{far}", f"1+{far}", f"+{far}+", "@n0", f"n0+ {far}", "+n1+1"])
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("d", HUB_LENGTHS)
def test_hub_as_the_last_of_a_300_node_frontier(gpu, d):
    """node 0 → 300 nodes; each lists one entry but the last, which lists d"""
    tg, distinct = hub_targets(301, d)
    n = 301 + distinct + 1
    src = [0] * 300 + list(range(1, 300)) + [300] * d
    dst = list(range(1, 301)) + [301 + (i % distinct) for i in range(299)] + tg
    c = Case(gpu, n, src, dst)
    c.check(["n0+", "n0+2", "n0+1", f"+{name_of(301)}", f"+{name_of(300 + distinct)}+", "@n300"])
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("d", [1, 63, 64, 65, 257, 5000])
def test_bottom_up_scan_finds_the_only_frontier_member(gpu, d, where):
    """node 1's in-list has d entries; only node 0 of them is ever in a frontier, and it stands first or last; node 1 → node 2"""
    others = list(range(3, 3 + d - 1))
    ins = [0] + others if where == "first" else others + [0]
    n = 3 + d - 1 + 1
    src = ins + [1]
    dst = [1] * d + [2]
    c = Case(gpu, n, src, dst)
    c.check(["n0+", "n0+1", "+n2", "+n2+", "@n0", f"+{name_of(n - 2)}+" if d > 1 else "n1+"])
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("width", [1, 63, 64, 65, 256, 257, 4097])
def test_frontier_widths_each_node_reached_from_two(gpu, width):
    """node 0 → a level of `width` nodes → two more such levels; node i of a level is listed by nodes i and i + 1 of the one before"""
    a, b, cc = 1, 1 + width, 1 + 2 * width
    n = 1 + 3 * width
    src, dst = [0] * width, list(range(a, a + width))
    for lo, hi in ((a, b), (b, cc)):
        for i in range(width):
            src += [lo + i, lo + (i + 1) % width]
            dst += [hi + i, hi + i]
    c = Case(gpu, n, src, dst)
    c.check(["n0+", "n0+2", f"+{name_of(cc)}", f"2+{name_of(cc + width - 1)}", f"+{name_of(b)}+", "@n0", f"@{name_of(b + width - 1)}",
             f"1+{name_of(b)}+1"])
    c.close()


@pytest.mark.gpu
def test_contested_claims_300_by_300(gpu):
    """node 0 → 300 nodes → each of them lists the same 300 nodes → each of those lists one sink"""
    a, b, sink = 1, 301, 601
    src = [0] * 300 + [a + i for i in range(300) for _ in range(300)] + list(range(b, b + 300))
    dst = list(range(a, a + 300)) + [b + j for _ in range(300) for j in range(300)] + [sink] * 300
    c = Case(gpu, 602, src, dst)
    c.check(["n0+", "n0+2", "+n601", "2+n601", "+n301+", "@n1", "1+n450+1", "n0+ +n601", "n0+,+n601", "not n1+"])
    c.close()


@pytest.mark.gpu
def test_path_of_2000_nodes_and_its_limits(gpu):
    n = 2000
    c = Case(gpu, n, np.arange(n - 1), np.arange(1, n))
    exprs = []
    for lim in ("0", "1", "2", "1999", "2000", ""):
        exprs += [f"n0+{lim}", f"{lim}+n1999", f"{lim}+n1000+{lim}"]
    c.check(exprs + ["@n1990", "1+n5+3 n7", "not n3+"])
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("group", [4, 16, 0])
def test_paths_around_the_group_size(gpu, group):
    """paths of G - 1, G and G + 1 steps with limits at the same three values, G the levels queued per read-back (0: the default)"""
    G = group or gpu.graph.SELECT_LEVELS_PER_SYNC
    modes = [(bu, str(group) if group else None) for bu in ("0", "1", "auto")]
    for steps in (G - 1, G, G + 1):
        n = steps + 1
        c = Case(gpu, n, np.arange(n - 1), np.arange(1, n))
        c.check([f"n0+{lim}" for lim in (G - 1, G, G + 1)] + ["n0+", f"+{name_of(steps)}", f"{G}+{name_of(steps)}", f"{G}+n1+{G}"], modes)
        c.close()


@pytest.mark.gpu
def test_levels_are_queued_in_groups(gpu):
    """the statistics of a call: level launches come in groups, one status read-back each; forcing bottom-up is counted"""
    n = 200
    c = Case(gpu, n, np.arange(n - 1), np.arange(1, n))
    saved = {k: os.environ.pop(k, None) for k in ("MN_SELECT_BOTTOM_UP", "MN_SELECT_LEVELS_PER_SYNC")}
    try:
        # 99 levels find a node; the first group that ends at or after the 99th reports a frontier without list entries
        for G, env in ((gpu.graph.SELECT_LEVELS_PER_SYNC, None), (8, "8"), (1, "1")):
            if env:
                os.environ["MN_SELECT_LEVELS_PER_SYNC"] = env
            c.g.select("n100+", names=index_of)
            st = c.g.select_stats
            groups = -(-99 // G)
            assert (st["rows"], st["levels"], st["launches"], st["syncs"], st["bottom_up_levels"]) == (100, 99, groups * G, groups, 0), G
        os.environ["MN_SELECT_LEVELS_PER_SYNC"] = "1"
        os.environ["MN_SELECT_BOTTOM_UP"] = "1"
        c.g.select("n0+10", names=index_of)
        st = c.g.select_stats
        assert (st["rows"], st["levels"], st["launches"], st["syncs"], st["bottom_up_levels"]) == (11, 10, 10, 10, 10)
        os.environ["MN_SELECT_BOTTOM_UP"] = "sometimes"
        with pytest.raises(gpu.hnsw.MuninnHipError, match="MN_SELECT_BOTTOM_UP"):
            c.g.select("n0+", names=index_of)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    c.close()


def random_digraph(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 501))
    e = int(rng.integers(n // 2, 4 * n))
    src, dst = rng.integers(0, n, e), rng.integers(0, n, e)
    k = max(1, e // 20)
    src[:k] = dst[:k]  # self-loops
    src[k:2 * k], dst[k:2 * k] = src[-k:], dst[-k:]  # rows that occur twice
    return n, src, dst


def random_expression(rng, n):
    def name():
        return "nosuch%d" % rng.randrange(3) if rng.random() < 0.03 else name_of(rng.randrange(n))

    def lim():
        return rng.choice(["", "", "0", "1", "2", "3"])

    def atom():
        kind = rng.randrange(5)
        x = name()
        return (x, f"{lim()}+{x}", f"{x}+{lim()}", f"{lim()}+{x}+{lim()}", f"@{x}")[kind]

    terms = []
    for _ in range(rng.randint(1, 8)):
        if rng.random() < 0.2:
            terms.append("not " + atom())
        else:
            terms.append(",".join(atom() for _ in range(rng.choice([1, 1, 2, 3]))))
    # a '+' that a blank and a name follow would open the next term: such a term gets a limit no walk here reaches
    return "  ".join(t + "999" if t.endswith("+") and i + 1 < len(terms) else t for i, t in enumerate(terms))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(20))
def test_random_digraphs_with_cycles(gpu, seed):
    n, src, dst = random_digraph(100 + seed)
    c = Case(gpu, n, src, dst)
    rng = random.Random(seed)
    x = name_of(int(src[len(src) // 2]))
    lims = ("", "0", "1", "2", "3")
    exprs = [f"{u}+{x}+{d}" for u in lims for d in lims] + [f"@{x}", f"@{name_of(rng.randrange(n))}"]
    exprs += [random_expression(rng, n) for _ in range(10)]
    c.check(exprs)
    c.close()


def test_random_expressions_are_well_formed_and_try_every_operator():
    """the generator of the test above, on the CPU: every text parses, and the operators and unknown names all occur"""
    rng = random.Random(0)
    ops, unknown = set(), 0
    for _ in range(200):
        expr = random_expression(rng, 300)
        prog = sm.parse(expr)
        ops |= {p[0] for p in prog}
        unknown += any(p[1] and p[1].startswith(b"nosuch") for p in prog)
    assert ops == set(range(8)) and 3 <= unknown <= 100


@pytest.mark.gpu
def test_names_long_unknown_name_and_a_hand_built_program(gpu):
    rows = [("raw.orders", "stg_orders"), ("raw.users", "stg_users"), ("stg_orders", "fct-orders"), ("stg_users", "fct-orders"),
            ("fct-orders", "report")]
    names = []
    for s, d in rows:
        names += [v for v in (s, d) if v not in names]
    src, dst = [names.index(s) for s, _ in rows], [names.index(d) for _, d in rows]
    g = gpu.graph.graph_from_edges(len(names), src, dst)
    node, depth, direction = g.select("+fct-orders", names=names)
    assert ([names[i] for i in node], depth.tolist(), direction) == (
        ["raw.orders", "stg_orders", "raw.users", "stg_users", "fct-orders"], [2, 1, 2, 1, 0], "ancestor")
    node, depth, direction = g.select("@stg_users raw.orders+1", names=names)
    assert sorted(names[i] for i in node) == sorted(names) and set(depth.tolist()) == {0} and direction == "selected"
    for expr in ("1+report+1", "not raw.users+", "stg_orders+,stg_users+"):
        want = sm.select_indices(len(names), src, dst, expr, names)
        got = g.select(expr, names=names)
        assert (got[0].tolist(), got[1].tolist(), got[2]) == want
    with pytest.raises(ValueError) as e:
        g.select("report " + "y" * 300 + "+ nosuch", names=names)
    assert e.value.args[0] == "graph_select: node '" + "y" * 235
    with pytest.raises(ValueError, match="^graph_select: node '12' not found$"):
        g.select("1 12", names=None)  # decimal names: 1 is a node, 12 is not
    assert g.select("5 1", names=None)[0].tolist() == [1, 5]
    for prog in ([(sm.DESCENDANTS, len(names), -1, -1)], [(sm.NODE, -1, -1, -1)], [(sm.NODE, 0, -1, -1), (sm.UNION, -1, -1, -1)],
                 [(sm.NODE, 0, -1, -1), (sm.NODE, 1, -1, -1)], [(99, 0, -1, -1)], []):
        with pytest.raises(gpu.hnsw.MuninnHipError, match="mn_graph_select"):
            g.select_program(prog)
    assert g.select_program([(sm.DESCENDANTS, 0, -1, -1)])[0].tolist() == [0, 1, 4, 5]  # the handle still answers
    g.close()
