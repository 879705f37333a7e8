"""The test-side model of the entity-resolution stages (tests/er_model.py) against what the compiled reference answered
(tests/golden/er.json.gz, written by scripts/gen_er_golden.py), and the recorded grid itself: a grid whose cases all give the
same clusters would let a wrong guard, a wrong cut or a wrong weight pass.  No device."""
import gzip
import json
import os

import numpy as np
import pytest

import er_model as em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "er.json.gz"), "rb") as f:
        return json.loads(f.read())


def test_model_equals_every_recorded_jaro_winkler_bit(golden):
    assert len(golden["jw"]) >= 600
    bad = [(a, b) for a, b, want in golden["jw"] if em.bits(em.jaro_winkler(bytes.fromhex(a), bytes.fromhex(b))) != want]
    assert not bad, bad[:3]


def test_recorded_pairs_are_the_fixed_list(golden):
    """the GPU tests run the device on the recorded strings; the list must still be the one that covers every length and class"""
    assert [(bytes.fromhex(a), bytes.fromhex(b)) for a, b, _ in golden["jw"]] == em.fixed_pairs()
    lens = {len(bytes.fromhex(a)) for a, _, _ in golden["jw"]}
    assert set(em.LENGTHS) | {4096} <= lens


def clusters(js):
    by = {}
    for key, cl in json.loads(js)["clusters"].items():
        by.setdefault(cl, []).append(key)
    return by


def test_grid_is_not_vacuous(golden):
    """What scripts/gen_er_golden.py asserts before it writes, asserted on the file.  The bridge cut: the reference's function
    cannot answer a case in which an edge exceeds the threshold — it writes its first bridge through a null pointer
    (src/llama_er.c:465-468, two arrays grown on one capacity counter) — so those cases are recorded from the reference's own
    graph_edge_betweenness and graph_leiden put together by the generator, which is held to the function's text on every case
    the function does answer; they are marked "composed"."""
    g = golden["grid"]["main"]
    sizes = sorted(len(v) for v in clusters(g["base"]["json"]).values())
    assert sizes[-1] >= 3 and sizes[0] == 1 and sizes.count(1) >= 5
    assert g["same_source"]["json"] != g["unguarded"]["json"]
    assert g["diff_type"]["json"] != g["unguarded"]["json"]
    assert g["same_source"]["json"] != g["diff_type"]["json"]
    assert g["unknown_guard"]["json"] == g["unguarded"]["json"] == g["base"]["json"] == g["chat_ignored"]["json"]
    assert g["eb_cut"]["json"] != g["eb_null"]["json"] and g["eb_cut"]["composed"]
    assert g["eb_none"]["json"] == g["eb_null"]["json"] and not g["eb_none"]["composed"]
    assert len({g["jw0"]["json"], g["jw05"]["json"], g["jw1"]["json"]}) > 1
    assert all(golden["branches"][b] > 0 for b in em.BRANCHES), golden["branches"]
    assert golden["grid"]["after_delete"]["base"]["json"] != g["base"]["json"]
    for state in golden["grid"].values():
        for case in state.values():
            assert list(json.loads(case["json"])["clusters"]) == [e[1] for e in golden["entities"]]  # keys in entity order


def test_candidates_keeps_first_appearance_and_smallest_distance():
    """the model's own reading of src/llama_er.c:237-284 on a case small enough to check by hand"""
    ent = [10, 20, 30, 40]
    ids = [[10, 20, 30], [10, 99, -1], [40, 20, 10], [-1, -1, -1]]
    ds = [[0.0, 0.25, 0.5], [0.125, 0.1, 0.0], [0.3, 0.2, 0.45], [0, 0, 0]]
    cnt = [3, 2, 3, 0]
    got = em.candidates(ent, ids, ds, cnt, 0.5)
    assert [(a, b) for a, b, _ in got] == [(0, 1), (0, 2), (2, 3), (1, 2)]
    assert [d for _, _, d in got] == [float(np.float32(x)) for x in (0.125, 0.45, 0.3, 0.2)]  # the doubles of the f32 distances


def test_cascade_branches():
    names = [b"Ann Lee", b"Ann Lee", b"ANN LEE", b"Anne Lee", b"Bob"]
    src = [b"a", b"a", b"b", b"", b"b"]
    cands = [(0, 1, 0.1), (0, 2, 0.1), (0, 3, 0.1), (0, 4, 0.1), (2, 4, 0.1)]
    hit = {}
    out = em.cascade(cands, names, src, None, 0.5, 0.8, hit)
    assert [(i, j) for i, j, _ in out] == [(0, 1), (0, 2), (0, 3)]
    assert out[0][2] == 1.0 and out[1][2] == 0.9
    assert out[2][2] == 0.5 * em.jaro_winkler(b"ann lee", b"anne lee") + (1.0 - 0.5) * (1.0 - 0.1)
    assert hit["exact"] == 1 and hit["lower"] == 1 and hit["jw"] == 3 and hit["dropped"] == 2
    assert [(i, j) for i, j, _ in em.cascade(cands, names, src, "same_source", 0.5, 0.8)] == [(0, 2), (0, 3)]
    assert [(i, j) for i, j, _ in em.cascade(cands, names, src, "diff_type", 0.5, 0.8)] == [(0, 1), (0, 3)]
