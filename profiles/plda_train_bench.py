#!/usr/bin/env python3
"""PLDA training at the reference's shape (include/xvec_plda.h, xvector_amd.plda): one statistics pass and four fits
(rank 50 / 100 / 150 / 200, 10 iterations each) on synthetic labelled x-vectors -- N ~ 400 000 rows of 512 (fp32, on the
device, as the extractor leaves them), 1211 classes of uneven size -- plus the numpy restatement of speechbrain's loop
(tests/plda_em_ref.py) for one rank-200 fit on the host's threads as the reference-side baseline.  Prints one JSON line.

    python3 profiles/plda_train_bench.py [--n-classes 1211] [--no-baseline]

`stats_call_*` time the library call alone between device events (its five launches); the rate quoted against it is a
lower bound of the scatter kernel's (whose own time is in a rocprofv3 kernel trace).  FLOP count: the algorithm's over the
upper triangle of 64 x 64 tiles; the fp64 peak is the vendor figure (78.6 TFLOP/s), not a rate measured on this shape."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import plda_em_ref as ref  # noqa: E402
from xvector_amd import hip, plda  # noqa: E402

PEAK_F64_TFLOPS = 78.6      # vendor figure, not measured here


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-classes", type=int, default=1211)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    x, labels, _ = ref.make_data(a.n_classes, a.dim, 150, sizes=(100, 560), seed=1)
    n, dim = x.shape
    xt = torch.from_numpy(x.astype(np.float32)).to(dev)
    torch.cuda.synchronize()

    plda.PldaStats(xt, labels)                                   # warm-up (code objects, allocator)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    stats_ms = []
    for _ in range(a.repeats):
        t0, t1 = ev(), ev()
        t0.record()
        st = plda.PldaStats(xt, labels)                          # ends in device-to-host copies: synchronous
        t1.record()
        t1.synchronize()
        stats_ms.append(t0.elapsed_time(t1))

    # the library call alone (no labels, no uploads, no copies back): its five launches between two events; the scatter
    # kernel's own time is in the rocprofv3 kernel trace
    classes, order, start = plda._labels(labels, n)
    C = classes.shape[0]
    f64 = dict(dtype=torch.float64, device=dev)
    outs = [torch.empty(dim, **f64), torch.empty(C, **f64), torch.empty((C, dim), **f64), torch.empty((dim, C), **f64),
            torch.empty((dim, dim), **f64)]
    wsb = int(hip.lib.xvec_plda_stats_workspace_bytes(n, dim, C))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    order_d = torch.from_numpy(order).to(dev)
    sp = start.ctypes.data_as(hip.C.POINTER(hip.C.c_int64))

    def call():
        rc = hip.lib.xvec_plda_stats(xt.data_ptr(), hip.PLDA_X_F32, n, dim, order_d.data_ptr(), sp, C, 1.0,
                                     *[o.data_ptr() for o in outs], ws.data_ptr(), wsb,
                                     torch.cuda.current_stream().cuda_stream)
        assert rc == 0, hip.lib.xvec_plda_last_error()
    call()
    torch.cuda.synchronize()
    call_ms = []
    for _ in range(a.repeats):
        t0, t1 = ev(), ev()
        t0.record()
        call()
        t1.record()
        t1.synchronize()
        call_ms.append(t0.elapsed_time(t1))

    tiles = (dim + 63) // 64
    scatter_flop = 2.0 * n * (64 * 64) * tiles * (tiles + 1) / 2
    n_tri = tiles * (tiles + 1) // 2
    bytes_read = n * 4 * (dim + 64 * (2 * n_tri - tiles))     # class sums once + each tile's strips (one on the diagonal)

    fits = {}
    for r in (50, 100, 150, 200):
        w0 = time.perf_counter()
        st.fit(r, 10)
        wall = time.perf_counter() - w0
        t = st.last_fit_timing
        fits[f"r{r}"] = {"wall_s": round(wall, 4), "device_s": round(t["device_s"], 4), "host_s": round(t["host_s"], 4)}

    res = {
        "workload": "plda_train", "n": int(n), "dim": int(dim), "n_classes": int(C), "nb_iter": 10, "x_dtype": "fp32",
        "build": hip.version(), "device": torch.cuda.get_device_name(dev),
        "stats_pass_ms_median": round(float(np.median(stats_ms)), 3),
        "stats_call_device_ms_median": round(float(np.median(call_ms)), 3),
        "stats_call_device_ms_min": round(float(np.min(call_ms)), 3),
        "scatter_gflop": round(scatter_flop / 1e9, 2),
        "stats_call_fp64_tflops_lower_bound": round(scatter_flop / (np.min(call_ms) * 1e-3) / 1e12, 2),
        "fp64_peak_tflops_vendor_unmeasured": PEAK_F64_TFLOPS,
        "stats_bytes_read_algorithmic": int(bytes_read),
        "fits": fits,
    }
    if not a.no_baseline:
        threads = os.environ.get("OMP_NUM_THREADS", "unset")
        w0 = time.perf_counter()
        ref.plda_em(x.astype(np.float32).astype(np.float64), labels, 200, 10)
        res["numpy_restatement_r200_s"] = round(time.perf_counter() - w0, 2)
        res["numpy_threads"] = threads
    print(json.dumps(res))


if __name__ == "__main__":
    main()
