"""tests/select_model.py and the library's selector parser against what the compiled reference's graph_select returned for
the grid below (tests/golden/select.json.gz, written by scripts/gen_select_golden.py).  CPU only: mn_select_parse touches no
device, and the model is the checker of tests/test_select.py and bench_select.py, so both are held to the recorded rows and
error strings here."""
import gzip
import json
import os
import random

import pytest

import select_model as sm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "select.json.gz")
LONG_NAME = "x" * 260  # the "not found" message is cut to 255 bytes


def golden():
    with gzip.open(GOLDEN, "rb") as f:
        return json.loads(f.read().decode())


def graph_cases():
    """name → the (src, dst) rows of an edge table, in row order"""
    return {
        # the chain a→b→c, with nodes whose names try the tokenizer: the keyword, '.', '-', a leading '_', a leading digit
        "words": [("a", "b"), ("b", "c"), ("not", "a"), ("m.x-1", "c"), ("_u", "a"), ("9z", "c"), (None, "a"), ("c", None)],
        "cyclic": [("a", "b"), ("b", "c"), ("c", "a"), ("c", "d"), ("d", "b"), ("z", "a")],
        # a diamond r→{a,b}→t, a duplicate row, a self-loop, a second root u, a tail t→y→z and a node w that only feeds y
        "dag": [("r", "a"), ("r", "b"), ("a", "t"), ("b", "t"), ("a", "t"), ("t", "t"), ("u", "b"), ("t", "y"), ("y", "z"), ("w", "y")],
        "numeric": [(1, 2), (2, 12), (12, 3), (3, 4), (12, 5), (7, 12), (5, 6), (6, 3), (4, 40)],
        "empty": [],
    }


def selectors():
    """name → the selector texts recorded for that table"""
    words = [
        "a", "c", "+c", "a+", "+b+", "1+c", "2+c", "a+1", "a+2", "a+0", "0+c", "0+b+0", "1+b+1", "1+c+1", "+a+1", "1+a+",
        # depth rules under a set operator
        "1+c b", "c+0 a", "a+0 c", "0+c a", "1+c+1 a", "1+c,+c", "a+1,a+", "not 1+c", "not a+0", "not 1+b+1",
        "@b", "@+b", "@b+", "@a", "@c", "@a b", "not @c", "+c,@a",
        # the keyword
        "not", "not,a", "a,not", "not a", "not not", "not  a", "a not b", "not a not b", "+not", "not+", "not +not+", " not ",
        "nota", "not_", "a not", "not ,a", "a, not", "not)", "not a,b",
        # digits and pluses
        "2+ c", "007+c", "7 +c", "2 + c", "a +c", "a+ c", "a + c", "c +2", "c+ 2", "c + 2", "a+b", "a++c", "a+1+c", "a+1 +c",
        "1 + b + 1", "+ c", "a +", "a+,c", "a+ ,c", "+c,a+", "a+1,c", "1+c+1,b", "9z", "+9z+", "9z+9", "9+9z", "9",
        # names
        "m.x-1", "m.x-1+", "+m.x-1", "_u", "_u+1", "m.x", ".a", "-a", "a.", "a-",
        # set operators
        "a b c", "a,b", "a,a", "a+,+c", "a+,+c b", "a b,c", "a,b c", "a+,+c,b", "a b c,c", "not a b", "b not a", "not a,a",
        "a\tb", "  a   b  ", "a+ b+ c+",
        # errors
        "", " ", "\t", "+", "@", ",", "a,", ",a", "a b,", "a,,b", "a$", "a $", "$a", "a(b)", "a;b", "(a)", "a|b", "a\nb",
        "+ +c", "@@a", "1+", "1++c", "+1+", "not not a", "not @", "a @", "a,+", "nosuch", "a nosuch other", "nosuch2,a",
        "a,nosuch3 nosuch4", "not nosuch5", "@nosuch6", "+nosuch7+", "3+nosuch8", "12", "a 12+", LONG_NAME, "a " + LONG_NAME + "+",
        "A",
    ]
    letters = ["+a+", "1+a+2", "1+a+3", "1+a", "a+3", "+a", "a+", "1+a+2 z", "1+a a+3", "+b+", "2+d+1", "@a", "@z", "@d", "z+", "+z",
               "z+1", "z+2", "not +a+", "+a+,z+", "0+a+0", "0+a+", "+a+0", "not 1+a+2", "1+a+1,b+"]
    dag = ["r", "+t", "r+", "+t+", "1+t+1", "@a", "@b", "@t", "@u", "@y", "@w", "@z", "@r", "@a u", "not @a", "t+1", "2+z", "3+z", "+z", "r+2",
           "u+", "+a+", "+b+", "a+,b+", "a+ b+", "+a,+b", "+y", "w+", "not w+", "r+1 u+1", "2+y+1", "t", "+t,r+", "1+t", "t+"]
    numeric = ["12", "12+", "+12+", "3+12", "12+3", "+12", "12+1", "1+12", "1+12+1", "12 3", "12,3", "12+,3+", "3 +12", "3+ 12",
               "12 +3", "40", "4 40", "+40", "040", "12+012", "@12", "@3", "not 12+", "1", "1+", "1+1", "1+1+1", "2+2+2", "99", "+99",
               "1 2 3 4 5 6 7 12 40", "6+"]
    return {"words": words, "cyclic": letters, "dag": dag, "numeric": numeric,
            "empty": ["a", "+a+", "@a", "nosuch", "a nosuch", "a$", "", "+", "a,", "not a"]}


def model_answer(rows, expr):
    try:
        return {"rows": [[i] + r for i, r in enumerate(sm.text_select(rows, expr))]}
    except sm.SelectError as e:
        return {"error": e.args[0].decode("utf-8", "replace")}


@pytest.mark.parametrize("name", sorted(graph_cases()))
def test_model_equals_the_recorded_rows_and_errors(name):
    rows, z = graph_cases()[name], golden()["select"][name]
    assert len(z) == len(selectors()[name])
    for expr, want in zip(selectors()[name], z):
        assert model_answer(rows, expr) == want, (name, expr)


def test_recorded_grid_is_not_vacuous():
    z = golden()["select"]
    at = lambda name, expr: z[name][selectors()[name].index(expr)]
    nodes = lambda a: {r[1] for r in a["rows"]}
    depth = lambda a: {r[1]: r[2] for r in a["rows"]}
    # the two passes of +x+ share a visited set: not the ancestors and the descendants computed apart
    assert depth(at("cyclic", "+a+")) == {"a": 0, "b": 2, "c": 1, "d": 3, "z": 1} and depth(at("cyclic", "a+"))["b"] == 1
    assert depth(at("cyclic", "1+a+2")) == {"a": 0, "b": 1, "c": 1, "z": 1}
    assert "d" in nodes(at("cyclic", "a+3")) and "d" not in nodes(at("cyclic", "1+a+3"))
    # a limit under a set operator is ignored unless it is 0; N+x+M keeps its own
    assert nodes(at("words", "1+c")) == {"b", "c", "m.x-1", "9z"} and "a" in nodes(at("words", "1+c b"))
    assert nodes(at("words", "a+0 c")) == {"a", "c"} and nodes(at("words", "a+1")) == {"a", "b"}
    assert nodes(at("words", "1+c+1 a")) == {"a", "b", "c", "m.x-1", "9z"}
    assert all(r[2] == 0 and r[3] == "selected" for r in at("words", "1+c b")["rows"])
    assert max(depth(at("dag", "@a")).values()) > 0 and depth(at("dag", "@a"))["t"] == 0
    assert at("words", "not")["rows"] == [[0, "not", 0, "self"]]
    assert at("words", LONG_NAME)["error"] == "graph_select: node '" + "x" * 235
    assert at("empty", "nosuch") == {"rows": []} and "error" in at("empty", "a$")
    assert at("words", "a nosuch other") == {"error": "graph_select: node 'nosuch' not found"}


def _program(parse, expr):
    try:
        return parse(expr)
    except ValueError as e:
        m = e.args[0]
        return m if isinstance(m, bytes) else m.encode("utf-8", "surrogateescape")


def test_library_parser_equals_the_model_on_the_recorded_grid(mn):
    for name, exprs in sorted(selectors().items()):
        for expr in exprs:
            assert _program(mn.graph.select_parse, expr) == _program(sm.parse, expr), (name, expr)


def test_library_parser_equals_the_model_on_random_strings(mn):
    rng = random.Random(20)
    alphabet = ["a", "b", "c", "1", "2", "+", "@", ",", "not", " "]
    programs = errors = 0
    for _ in range(2000):
        expr = "".join(rng.choice(alphabet) for _ in range(rng.randint(1, 12)))
        got = _program(mn.graph.select_parse, expr)
        assert got == _program(sm.parse, expr), expr
        programs += isinstance(got, list)
        errors += isinstance(got, bytes)
    assert programs > 200 and errors > 200  # both sides of the grammar are tried


def test_library_parser_on_bytes_the_reference_cannot_be_asked_about(mn):
    """depths beyond INT_MAX saturate (the reference's int overflows there); a byte that is no UTF-8 is an unexpected character"""
    assert mn.graph.select_parse("99999999999+a+2147483648") == [(sm.BOTH, b"a", sm.INT_MAX, sm.INT_MAX)]
    assert mn.graph.select_parse("2147483647+a") == [(sm.ANCESTORS, b"a", sm.INT_MAX, -1)]
    for raw in (b"a\xff", b"\xe9", b"a \xc3\xa9+"):
        assert _program(mn.graph.select_parse, raw) == _program(sm.parse, raw)
    assert _program(mn.graph.select_parse, b"a\xff") == b"graph_select: unexpected character '\xff' at position 1"
