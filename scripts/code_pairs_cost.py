"""Times the two launches of ONE mmg_code_pair_hist call (include/mmg.h; csrc/kernels_pairs.h) on synthetic rows, between device
synchronisations.  (The cost inside a dev evaluation: scripts/eval_profile_cost.py --mode codes | topsim.)

  python scripts/code_pairs_cost.py --rows N [--steps S] [--bins K] [--feat F] [--numpy] [--calls N] [--warmup W] [--label L] [--lib SO]

N rows of codes with W = 32, T = 10; the first S steps are compared (default: all 10), K bins (default 64), an |N(0, 1)| meaning matrix
of F columns (default 512).  The shape decides the histogram's route: 2 (32 S + 1) K counters in the workgroup's LDS where they fit,
else global atomics (--lib: another build of the library, e.g. with -DMMG_PAIR_DYN_BYTES=40960, for an A/B of the two routes).
--numpy: also commstats.pair_hist_np on the same rows on this host, once, for scale, and how far the two histograms are apart.  Prints one JSON line: label, median / min / max in ms."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, required=True)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--bins", type=int, default=64)
ap.add_argument("--feat", type=int, default=512)
ap.add_argument("--numpy", action="store_true")
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--label", default="")
ap.add_argument("--lib", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from multimodalgame_amd import _lib, commstats  # noqa: E402

if args.lib:
    _lib.LIB_PATH = os.path.abspath(args.lib)
T, W, N, S, K, F = 10, 32, args.rows, args.steps, args.bins, args.feat
rng = np.random.RandomState(0)
tsel = rng.randint(0, T, N)
codes = rng.randint(0, 1 << 32, (N, 2, T, 1), dtype=np.uint64).astype(np.uint32)
codes *= (np.arange(T)[None, :] <= tsel[:, None]).astype(np.uint32)[:, None, :, None]
meta = np.stack([tsel, rng.randint(0, 30, N)], 1).astype(np.int32)
x = np.abs(rng.randn(N, F)).astype(np.float32)
lib = _lib.load()
dev = torch.device("cuda:0")
cd, mt, xd = torch.from_numpy(codes.view(np.int32)).to(dev), torch.from_numpy(meta).to(dev), torch.from_numpy(x).to(dev)
inv = torch.empty(N, dtype=torch.float32, device=dev)
hist = torch.zeros(int(lib.mmg_code_pair_hist_count(S, W, K)), dtype=torch.int64, device=dev)
p = lambda t: C.c_void_p(t.data_ptr())
st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
times = []
for i in range(args.warmup + args.calls):
    hist.zero_()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _lib.check(lib.mmg_code_pair_hist(p(cd), p(mt), N, T, W, 0, 0, S, p(xd), F, F, p(inv), K, p(hist), st))
    torch.cuda.synchronize()
    if i >= args.warmup:
        times.append(1e3 * (time.perf_counter() - t0))
out = dict(label=args.label or "pair_hist_N%d_S%d_K%d" % (N, S, K), calls=len(times), median_ms=float(np.median(times)),
           min_ms=float(min(times)), max_ms=float(max(times)), rows=N, F=F, W=W, T=T, steps=S, bins=K, pairs=int(hist[2]),
           counters=2 * (S * W + 1) * K)
if args.numpy:
    t0 = time.perf_counter()
    want = commstats.pair_hist_np(codes, meta, x, 0, 0, S, K, W=W)
    out["numpy_ms"] = 1e3 * (time.perf_counter() - t0)
    got = commstats.parse_pair_hist(hist.cpu().numpy(), S, W, K)["hist"]
    ref = commstats.parse_pair_hist(want, S, W, K)["hist"]
    out["hamming_marginals_equal"] = bool(np.array_equal(got.sum(2), ref.sum(2)))
    out["pairs_in_another_bin"] = int(np.abs(got.cumsum(2) - ref.cumsum(2)).sum())
print(json.dumps(out))
