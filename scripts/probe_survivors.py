"""The filtered batch search (k_beam<SSE, 1, LP>) on the headline index (1M x 768 gaussian, cosine, 10k queries, ef 128):
  probe_survivors.py phase   per-expansion phase times with shadow pass and exact walk apart, and the histogram of filter passes
                             by survivors, from the -DMN_PHASE_TIMING build (scripts/build_phase_lib.py), for each layout
  probe_survivors.py occ     kernel_ms of the product library by wavefronts per SIMD (MN_LDS_PAD_BYTES lowers residency without a
                             rebuild) and layout (MN_SURVIVOR_LANES), three interleaved trials
  probe_survivors.py prof    four launches of the product library and nothing else after the build (for rocprofv3 runs)
usage: probe_survivors.py phase|occ|prof [N] [dim]"""
import ctypes as C, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import muninn_amd
pkg = muninn_amd.pkg
mode = sys.argv[1]
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
D = int(sys.argv[3]) if len(sys.argv) > 3 else 768
NQ, K, EF = 10_000, 10, 128
if mode == "phase":
    pkg.hnsw.LIB = os.path.join(ROOT, "scripts", "_phase", "libmuninn_hip.so")
L = pkg.hnsw.lib()
X = np.random.default_rng(42).standard_normal((N, D), dtype=np.float32)
Q = np.random.default_rng(43).standard_normal((NQ, D), dtype=np.float32)
g = pkg.HnswIndex(D, "cosine", 16, 200)
t = time.perf_counter(); assert g.build(np.arange(1, N + 1, dtype=np.int64), X) == 0; g.sync()
print(f"built {N}x{D} in {time.perf_counter() - t:.1f}s", flush=True)
dq = g.dev_malloc(Q.nbytes); g.dev_upload(dq, Q)
di, dd, dc = g.dev_malloc(NQ * K * 8), g.dev_malloc(NQ * K * 4), g.dev_malloc(NQ * 4)
def launch(lanes=None, pad=0, filt=True):
    for k, v in (("MN_SURVIVOR_LANES", lanes), ("MN_LDS_PAD_BYTES", pad or None), ("MN_LOWPREC_FILTER", None if filt else 0)):
        if v is None: os.environ.pop(k, None)
        else: os.environ[k] = str(v)
    g.search_batch_dev(dq, NQ, K, EF, di, dd, dc)
    return g.last_launch()
if mode == "phase":
    L.mn_debug_phase_kernels.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    def phases():
        a = (C.c_ulonglong * 16)()
        assert L.mn_debug_phase_kernels(a, 1) == 0
        return np.array(list(a), np.float64)
    # pad 5700: 3 wavefronts per SIMD, what the kernel ran at before it fitted 128 VGPRs
    for tag, lanes, pad in (("4 lanes per row, 3 waves/SIMD", 4, 5700), ("4 lanes per row", 4, 0), ("8 lanes", 8, 0), ("16 lanes", 16, 0), ("automatic", None, 0)):
        launch(lanes, pad); phases()
        st = launch(lanes, pad); p = phases()
        nexp, us = max(p[5], 1), p / 100.0
        print(f"{tag}: kernel {st['last_kernel_ms']:.2f} ms (timers on); expansions {p[5]:.0f}; per expansion: pop {us[0] / nexp:.2f} us, "
              f"row+visited {us[1] / nexp:.2f}, shadow pass {us[8] / nexp:.2f}, exact walk {us[2] / nexp:.2f}, pushes {us[3] / nexp:.2f} "
              f"(sum {(us[0] + us[1] + us[2] + us[3] + us[8]) / nexp:.2f} us); rows by lanes 4/8/16: {st['last_n_rows_lanes4']} / "
              f"{st['last_n_rows_lanes8']} / {st['last_n_rows_lanes16']}", flush=True)
    tot = max(p[14], 1)
    print(f"filter passes {p[14]:.0f} ({p[14] / nexp:.3f} per expansion), candidates per pass {p[15] / tot:.2f}; passes by survivors: "
          + ", ".join(f"{n} {p[9 + i]:.0f} ({100 * p[9 + i] / tot:.1f} %)" for i, n in enumerate(("0", "1-4", "5-8", "9-16", ">16"))), flush=True)
elif mode == "prof":
    for i in range(4):
        print(f"launch {i + 1}: kernel_ms {launch()['last_kernel_ms']:.2f}", flush=True)
else:
    cfgs = [("4 waves/SIMD", 0), ("3 waves/SIMD", 5700), ("2 waves/SIMD", 11000)]
    launch(); launch(4)
    for trial in range(3):
        for tag, pad in cfgs:
            for lanes in (4, None):
                st = launch(lanes, pad)
                print(f"trial {trial + 1}  {tag} (MN_LDS_PAD_BYTES={pad})  layout {'4 lanes' if lanes else 'automatic'}: kernel_ms {st['last_kernel_ms']:.2f}  "
                      f"n_dist {st['last_n_dist']} n_exp {st['last_n_expanded']} exact rows {st['last_n_exact_rows']} by lanes 4/8/16 "
                      f"{st['last_n_rows_lanes4']}/{st['last_n_rows_lanes8']}/{st['last_n_rows_lanes16']}", flush=True)
        st = launch(None, 0, filt=False)
        print(f"trial {trial + 1}  filter off: kernel_ms {st['last_kernel_ms']:.2f}", flush=True)
g.close()
