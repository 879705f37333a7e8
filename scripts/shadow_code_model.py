"""CPU model of the shadow filter's rejection power by code width (no GPU): which share of the candidates the layer-0 search
evaluates once its results are full survives the bound of DESIGN.md §3.1 (cosine, E doubled, gamma_{ld+8}, evaluated in f64) when
the shadow is fp16 under a power-of-two scale (the format up to round 6) or a uniform b-bit code x~ = rint(x / s) s,
s = max|x| / (2^(b-1) - 1) per row (10 bits: mn_device.hpp).  The index is built by the oracle with insert_batch in
mn_hnsw_build's schedule (M 16, efC 200, cosine); layer 0 is searched here with the reference's loop (heapq, ef 128, patience
ef / 4) and f64 distances.  usage: shadow_code_model.py [dataset] [N] [queries] [dim]"""
import heapq, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import gen_vectors
from oracle import orc
dataset = sys.argv[1] if len(sys.argv) > 1 else "gaussian"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 60_000
NQ = int(sys.argv[3]) if len(sys.argv) > 3 else 100
D = int(sys.argv[4]) if len(sys.argv) > 4 else 768
EF, BITS = 128, (12, 11, 10, 9, 8)
X, Q = gen_vectors(N, D, 42, dataset), gen_vectors(NQ, D, 43, dataset)
ids = np.arange(1, N + 1, dtype=np.int64)
o = orc.Oracle(D, "cosine", 16, 200)
pos = 0
while pos < N:  # mn_hnsw_build: grow_div 16, max_batch 8192
    b = max(1, min(o.node_count // 16, 8192, N - pos))
    assert o.insert_batch(ids[pos:pos + b], X[pos:pos + b]) == 0
    pos += b
buf = np.empty(4096, np.int64)
def nbrs(i, l):
    return buf[:o._neighbors(int(i), l, buf)] - 1  # ids are slot + 1
X64 = X.astype(np.float64)
xn = np.linalg.norm(X64, axis=1)
def coded(bits):  # (x~, r_x) of every row
    if bits == 16:
        e = np.floor(np.log2(np.abs(X).max(axis=1))) - 14
        Xt = np.ldexp(np.ldexp(X, -e[:, None].astype(np.int32)).astype(np.float16).astype(np.float32), e[:, None].astype(np.int32))
    else:
        s = (np.abs(X).max(axis=1) / np.float32(2 ** (bits - 1) - 1)).astype(np.float32)[:, None]
        Xt = np.rint(X / s).astype(np.float32) * s
    Xt = Xt.astype(np.float64)
    return Xt, np.linalg.norm(X64 - Xt, axis=1)
codes = {b: coded(b) for b in (16,) + BITS}
g = (D + 8) * 2.0 ** -24 / (1 - (D + 8) * 2.0 ** -24)
surv, exact, total = {b: 0 for b in codes}, 0, 0
for q in Q.astype(np.float64):
    qn = np.linalg.norm(q)
    dist = lambda i: 1.0 - (X64[i] @ q) / (xn[i] * qn)
    cur, l = o.entry_point - 1, o.max_level
    while l > 0:  # greedy descent
        best, moved = dist(cur), True
        while moved:
            moved = False
            for nb in nbrs(cur + 1, l):
                dn = dist(nb)
                if dn < best:
                    best, cur, moved = dn, nb, True
        l -= 1
    d0 = dist(cur)
    cand, res, seen, stale = [(d0, cur)], [(-d0, cur)], {cur}, 0
    while cand:
        dc, node = heapq.heappop(cand)
        if len(res) >= EF and (dc > -res[0][0] or stale >= max(EF // 4, 10)):
            break
        new = [nb for nb in nbrs(node + 1, 0) if nb not in seen]
        seen.update(new)
        improved = False
        filt = bool(new) and len(res) >= EF
        if filt:  # one filter pass: every bound is held against the worst result at its start
            w0, nw = -res[0][0], np.array(new)
            total += len(new)
            for b, (Xt, rx) in codes.items():
                A = Xt[nw] @ q
                E = 2.0 * (qn * (rx[nw] + g * (2.0 * xn[nw] + rx[nw])))
                surv[b] += int((1.0 - np.maximum(A + E, 0.0) / (qn * xn[nw]) < w0).sum())
        for nb in new:
            dn = dist(nb)
            if filt:
                exact += dn < w0
            if len(res) < EF or dn < -res[0][0]:
                heapq.heappush(cand, (dn, nb))
                (heapq.heappush if len(res) < EF else heapq.heapreplace)(res, (-dn, nb))
                improved = True
        stale = 0 if improved else stale + 1
print(f"{dataset}, N {N}, {NQ} queries, dim {D}: {total} filtered candidates; d < worst0 {exact / total:.4f}; survivors: "
      + ", ".join(f"{'fp16' if b == 16 else str(b) + '-bit'} {surv[b] / total:.4f}" for b in codes)
      + "; mean r_x/|x|: " + ", ".join(f"{'fp16' if b == 16 else str(b) + '-bit'} {np.mean(codes[b][1] / xn):.1e}" for b in codes))
