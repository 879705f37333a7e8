"""Test-side model of the reference's entity-resolution middle stages: jaro_winkler (src/string_sim.c:11-96), the candidate loop
with its de-duplication (src/llama_er.c:237-284) and the type guard + scoring cascade (:295-332), restated in Python.  Python
floats are IEEE doubles and nothing here is fused, so the f64 tails come out with the reference's bits (tests/test_er_model.py
holds jaro_winkler against bits recorded from the compiled reference).  CHECKER ONLY: the product never imports this."""
import struct

import numpy as np


def bits(x):
    """the 64 bits of a double as an int"""
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def lower(s: bytes) -> bytes:
    """tolower in the C locale, byte by byte (src/llama_er.c:48-54)"""
    return bytes(c + 32 if 65 <= c <= 90 else c for c in s)


def jaro_winkler(s1: bytes, s2: bytes) -> float:
    len1, len2 = len(s1), len(s2)
    if len1 == 0 and len2 == 0:
        return 1.0
    if len1 == 0 or len2 == 0:
        return 0.0
    if s1 == s2:
        return 1.0
    match_dist = max(len1, len2) // 2 - 1
    if match_dist < 0:
        match_dist = 0
    m1 = [False] * len1
    m2 = [False] * len2
    matches = 0
    for i in range(len1):
        lo = max(0, i - match_dist)
        hi = min(len2, i + match_dist + 1)
        for j in range(lo, hi):
            if m2[j] or s1[i] != s2[j]:
                continue
            m1[i] = m2[j] = True
            matches += 1
            break
    if matches == 0:
        return 0.0
    transpositions = 0
    k = 0
    for i in range(len1):
        if not m1[i]:
            continue
        while not m2[k]:
            k += 1
        if s1[i] != s2[k]:
            transpositions += 1
        k += 1
    jaro = (matches / len1 + matches / len2 + (matches - transpositions / 2.0) / matches) / 3.0
    prefix = 0
    for i in range(min(len1, len2, 4)):
        if s1[i] == s2[i]:
            prefix += 1
        else:
            break
    return jaro + prefix * 0.1 * (1.0 - jaro)


def candidates(ent_ids, nbr_ids, nbr_dists, counts, dist_threshold):
    """[(r1, r2, dist)] as the reference's loop leaves its array: entities in order, each list in order, the three tests, then the
    scan for an earlier (lo, hi) — here through a dict of the positions, which finds what the linear scan finds, a pair being
    in the array at most once — lowering its distance, else an append.  dist is the double of the f32 distance."""
    index_of = {int(r): i for i, r in enumerate(ent_ids)}  # rid_to_idx: the last entity wins, as its fill loop has it
    out, where = [], {}
    nbr_dists = np.asarray(nbr_dists, np.float32)
    for i in range(len(ent_ids)):
        c = int(counts[i])
        if c <= 0:
            continue
        for p in range(min(c, np.shape(nbr_ids)[1])):
            nid = int(nbr_ids[i][p])
            dist = float(nbr_dists[i][p])
            if nid == int(ent_ids[i]):
                continue
            if dist > dist_threshold:
                continue
            if nid not in index_of:
                continue
            j = index_of[nid]
            lo, hi = (i, j) if i < j else (j, i)
            at = where.get((lo, hi))
            if at is not None:
                if dist < out[at][2]:
                    out[at][2] = dist
            else:
                where[(lo, hi)] = len(out)
                out.append([lo, hi, dist])
    return [tuple(c) for c in out]


BRANCHES = ("guard_same_source", "guard_diff_type", "exact", "lower", "jw", "kept", "dropped")


def cascade(cands, names, sources, type_guard, jw_weight, match_threshold, branches=None):
    """[(r1, r2, weight)] of src/llama_er.c:295-332.  names: bytes per entity; sources: bytes per entity (b"" = none) or None;
    type_guard: "same_source" | "diff_type" | anything else.  branches (a dict, optional) counts the ways taken."""
    hit = branches if branches is not None else {}
    for b in BRANCHES:
        hit.setdefault(b, 0)
    low = [lower(n) for n in names]
    out = []
    for i, j, dist in cands:
        si = sources[i] if sources is not None else b""
        sj = sources[j] if sources is not None else b""
        if type_guard == "same_source":
            if si and sj and si == sj:
                hit["guard_same_source"] += 1
                continue
        elif type_guard == "diff_type":
            if si and sj and si != sj:
                hit["guard_diff_type"] += 1
                continue
        cosine_sim = 1.0 - dist
        if names[i] == names[j]:
            score = 1.0
            hit["exact"] += 1
        elif low[i] == low[j]:
            score = 0.9
            hit["lower"] += 1
        else:
            jw = jaro_winkler(low[i], low[j])
            score = jw_weight * jw + (1.0 - jw_weight) * cosine_sim
            hit["jw"] += 1
        if score >= match_threshold:
            out.append((i, j, score))
            hit["kept"] += 1
        else:
            hit["dropped"] += 1
    return out


# ───────────────────────── the fixed pair list of tests/golden/er.json.gz ─────────────────────────

LENGTHS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257)


def rand_name(rng, n, alphabet):
    return bytes(alphabet[i] for i in rng.integers(0, len(alphabet), n)) if n else b""


def swap_adjacent(s: bytes, at):
    b = bytearray(s)
    for i in at:
        if i + 1 < len(b):
            b[i], b[i + 1] = b[i + 1], b[i]
    return bytes(b)


def fixed_pairs():
    """[(a, b)]: what scripts/gen_er_golden.py records the reference's jaro_winkler for.  Lengths around every switch of the
    device code (window 0 up to 3 bytes, the 64-byte lane path, the 64-byte ballot steps, the 4096-byte limit), alphabets of 2 to
    4 letters so that matches and transpositions are dense, the full byte range, and the content classes that take the early
    exits; every pair also in the other argument order."""
    rng = np.random.default_rng(20240611)
    ab = [b"ab", b"abc", b"abcd"]
    full = bytes(range(1, 256))
    out = []
    for la in LENGTHS:
        for lb in LENGTHS:
            al = ab[(la + lb) % 3]
            out.append((rand_name(rng, la, al), rand_name(rng, lb, al)))
    for n in LENGTHS[1:]:
        s = rand_name(rng, n, full)
        out.append((s, s))                                            # identical
        out.append((s, rand_name(rng, n, full)))                      # full byte range
        out.append((s, swap_adjacent(s, range(0, n, 3))))             # adjacent swaps
        out.append((rand_name(rng, n, b"ab"), rand_name(rng, n, b"xy")))  # no common byte
        out.append((b"a" * n, b"a" * (n + 3)))                        # repeated bytes
        out.append((s.upper(), s.lower()))
    out += [(b"aaaa", b"aaaaaaa"), (b"", b""), (b"", b"abc"), (b"MARTHA", b"MARHTA"), (b"DIXON", b"DICKSONX"), (b"DWAYNE", b"DUANE")]
    base = rand_name(rng, 40, b"abcd")
    for p in range(6):                                                # common prefixes of 0 .. 5 bytes
        other = bytearray(rand_name(rng, 40, b"abcd"))
        other[:p] = base[:p]
        if p < 40:
            other[p] = ord("z")
        out.append((base, bytes(other)))
    big = rand_name(rng, 4096, b"ab")
    out.append((big, swap_adjacent(big, range(0, 4096, 5))))
    out.append((big, rand_name(rng, 4096, b"ab")))
    out.append((rand_name(rng, 4096, full), rand_name(rng, 70, full)))
    out.append((rand_name(rng, 4096, b"abc"), b""))
    return out + [(b, a) for a, b in out]
