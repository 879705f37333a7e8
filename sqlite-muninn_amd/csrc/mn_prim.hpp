// mn_prim.hpp — rocPRIM's two-phase call over a temporary the handle keeps.  Included by the graph files that use rocPRIM.
#pragma once
#include "mn_graph_int.hpp"

// `call(tmp, bytes)` is one rocPRIM device function with everything but its first two arguments bound: asked with a null
// temporary for the size it wants, then run on `st` with `tmp` grown to that size if it must be (after `st` has drained:
// an earlier call may still be using the old one).  `what` names the rocPRIM function, `who` the entry point.
template <typename Call> int prim_run(const char *who, const char *what, DevBuf<char> &tmp, hipStream_t st, Call call) {
    size_t bytes = 0;
    if (call(nullptr, bytes) != hipSuccess) {
        gset_err("%s (size query) failed", what);
        return -1;
    }
    if (bytes > tmp.cap) {
        GCHK(hipStreamSynchronize(st));
        if (tmp.fit(gset_err, who, bytes))
            return -1;
    }
    if (call((void *)tmp.p, bytes) != hipSuccess) {
        gset_err("%s failed", what);
        return -1;
    }
    return 0;
}
