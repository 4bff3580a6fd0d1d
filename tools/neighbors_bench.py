#!/usr/bin/env python3
"""What the neighbour module costs on the MI355X: writes profiles/neighbors_cost.json (or --out).

* ``topk`` at M = N = 16 384, k = 10, cosine, against ``torch.topk(normalize(Q) @ normalize(K).T, 10)`` on the same machine: both
  times and both peak allocations above the inputs;
* ``topk`` at M = N = 131 072 (the torch form would need a 64 GiB matrix): time and achieved fp32 TFLOP/s (2 M N 768 over the time),
  with the exact-fp32 GEMM (``loco_op_gemm``) on 16 384 x 16 384 x 768 beside it;
* one k-means round (assignment, inertia, centre update) at N = 131 072, C = 18.

Device events around the work, one warm-up, the median of 9, clocks as found.  No bar is set on any of these figures."""
import argparse
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
L = importlib.import_module("loco-asr_amd._lib")
nb = importlib.import_module("loco-asr_amd.neighbors")

REPS = 9
D = 768


def median_ms(fn, reps=REPS):
    """Median over `reps` of the device time of fn(), each between two events, after one warm-up."""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return sorted(times)[len(times) // 2], min(times), max(times)


def peak_bytes(fn):
    """Peak of torch's allocator during fn() above what was allocated before it."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return int(peak)


def latent_data(rows, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    W = torch.randn(6, D, device="cuda", generator=g)
    return torch.randn(rows, 6, device="cuda", generator=g) @ W / 6 ** 0.5 + 0.3 * torch.randn(rows, D, device="cuda", generator=g)


def gemm_f32(A, W, C):
    M, N = A.shape[0], W.shape[0]
    L.check(L.load().loco_op_gemm(A.data_ptr(), D, W.data_ptr(), D, None, None, N, C.data_ptr(), N, M, N, D, 0, 1, 1, 0, 0, 0, 0,
                                  torch.cuda.current_stream().cuda_stream))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbors_cost.json"))
    ap.add_argument("--small", type=int, default=16384)
    ap.add_argument("--large", type=int, default=131072)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("neighbors_bench: needs the GPU; nothing is measured without one")
    res = {"device": torch.cuda.get_device_name(0), "reps": REPS, "timing": "device events, one warm-up, median of 9, clocks as found"}

    n = args.small
    Q, K = latent_data(n, 1), latent_data(n, 2)
    fused = lambda: nb.topk(Q, K, k=10, metric="cosine")  # noqa: E731
    norm = torch.nn.functional.normalize
    dense = lambda: torch.topk(norm(Q) @ norm(K).T, 10)  # noqa: E731
    a, b = fused(), dense()
    agree = float((a.indices.long() == b.indices).float().mean())
    t_f, t_d = median_ms(fused), median_ms(dense)
    res["topk_small"] = {"M": n, "N": n, "k": 10, "metric": "cosine", "fused_ms": t_f[0], "fused_ms_min_max": t_f[1:], "torch_ms": t_d[0],
                         "torch_ms_min_max": t_d[1:], "fused_tflops": 2.0 * n * n * D / t_f[0] / 1e9, "fused_peak_bytes": peak_bytes(fused),
                         "torch_peak_bytes": peak_bytes(dense), "index_agreement_with_torch": agree,
                         "torch_form": "torch.topk(normalize(Q) @ normalize(K).T, 10)"}
    del a, b
    C = torch.empty(n, n, device="cuda")
    t_g = median_ms(lambda: gemm_f32(Q, K, C))
    res["gemm_f32"] = {"M": n, "N": n, "K": D, "ms": t_g[0], "ms_min_max": t_g[1:], "tflops": 2.0 * n * n * D / t_g[0] / 1e9,
                       "what": "loco_op_gemm, exact fp32 MFMA, the M x N result written"}
    del C, Q, K
    torch.cuda.empty_cache()

    n = args.large
    X = latent_data(n, 3)
    fused = lambda: nb.topk(X, X, k=10, metric="cosine")  # noqa: E731
    t_l = median_ms(fused)
    res["topk_large"] = {"M": n, "N": n, "k": 10, "metric": "cosine", "ms": t_l[0], "ms_min_max": t_l[1:], "tflops": 2.0 * n * n * D / t_l[0] / 1e9,
                         "peak_bytes": peak_bytes(fused), "slab_rows": nb.slab_rows(n, n, 10, nb.SCRATCH_CAP),
                         "torch_form_matrix_bytes": 4 * n * n}

    init = nb.draw_init(n, 18, 0)

    def wall_ms(iters):  # host clock around work that ends in a synchronise: a round reads the inertia back
        def once():
            t0 = time.perf_counter()
            nb.kmeans(X, n_clusters=18, iters=iters, init=init)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        once()
        return sorted(once() for _ in range(REPS))[REPS // 2]

    t1, t3 = wall_ms(1), wall_ms(3)
    res["kmeans_round"] = {"N": n, "C": 18, "ms_per_round": (t3 - t1) / 2.0, "ms_iters_1": t1, "ms_iters_3": t3,
                           "what": "host clock, synchronised: (kmeans(iters=3) - kmeans(iters=1)) / 2 = one assignment, inertia read-back and centre update"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
