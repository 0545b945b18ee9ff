"""Which launches a minibatch enqueues, for comparing two builds of libmmg.so (a host-side change must leave the list alone).

  rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python scripts/launch_trace.py CASE MODE [--lib libmmg_other.so]
  python scripts/launch_trace.py --list DIR

The first form runs two minibatches of one case in a fresh process (environment switches come from the caller's environment);
MODE is one of MODES or `all` (every mode in turn, each on an engine of its own; a mode the library refuses is reported and skipped).  The second form prints the library's kernels
of the trace under DIR in dispatch order: name, grid, workgroup size, LDS bytes.  Kernel trace only -- never with counters.

--lib names a second build inside multimodalgame_amd/ (git-ignored like libmmg.so).  To make the other commit's library, export
that commit to a scratch directory and build it there, then copy it beside libmmg.so under another name:
  git archive COMMIT | tar -x -C /tmp/other && (cd /tmp/other && python -m multimodalgame_amd.build) &&
  cp /tmp/other/multimodalgame_amd/libmmg.so multimodalgame_amd/libmmg_parent.so"""
import csv
import glob
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# engine keywords over bench.C2 and the batch: the shapes of tests/test_option_branches_cpu.py / tests/test_hip_configs.py
C4 = dict(h_dim=1024, w_dim=256, max_exchange=4)
MC3 = dict(n_classes=200, use_binary=False, fixed_exchange=True, max_exchange=4, entropy_s=None, entropy_sen=None, entropy_rec=None)
CASES = {
    "c1": (dict(), 16),
    "c1-fixed": (dict(fixed_exchange=True, max_exchange=4), 16),
    "tiny": (dict(n_classes=5, feat_dim=16, h_dim=8, w_dim=6, rec_hidden=5, wv_dim=7, bas_hidden=9, max_exchange=5, top_k=2), 8),
    "c1-wv300": (dict(wv_dim=300), 16),
    "c4": (C4, 16),
    "c4-256": (C4, 256),                       # consecutive role launches
    "c4-1024": (C4, 1024),                     # the per-step fall-back
    "c4-R256": (dict(C4, rec_hidden=256), 16),
    "c1-D200": (dict(n_classes=200), 16),
    "mc3": (MC3, 16),
    "mc3p": (MC3, 512),                        # the smallest batch mc3p_shape accepts
}
MODES = ("fused", "phased", "dp0", "dp1", "eval", "evalsteps")


def run(case, mode):
    import torch
    import bench
    from multimodalgame_amd.agents import init_state_dicts
    from multimodalgame_amd.engine import Engine
    kw, B = CASES[case]
    cfg = dict(bench.C2, **kw)
    eng = Engine(batch=B, **cfg)
    eng.load_state_dicts(init_state_dicts(eng, seed=0))
    feats, target, desc = bench.synthetic_dataset(2 * B, cfg["n_classes"], cfg["feat_dim"], cfg["wv_dim"])
    x, t, d = (torch.from_numpy(a).to(eng.device) for a in (feats, target, desc))
    if mode == "evalsteps":
        eng.eval_steps(x, t, d, 2, cfg["top_k"], eng.eval_acc())
    for i in range(0 if mode == "evalsteps" else 2):
        xi, ti = x[i * B:(i + 1) * B], t[i * B:(i + 1) * B]
        if mode == "fused":
            eng.train_step(xi, ti, d, seed=11 + i)
        elif mode == "phased":
            eng.forward(xi, ti, d, seed=11 + i, train=True, run_all=True)
            eng.loss_stats()
            eng.backward(xi, ti, d)
            eng.clip_step()
        elif mode in ("dp0", "dp1"):
            eng.dp_train_step(xi, ti, d, seed=11 + i, full_tape=mode == "dp1", reduce=False)
        else:
            eng.forward(xi, ti, d, train=False)
    torch.cuda.synchronize()
    eng.check_sync()


def listing(root):
    rows = []
    for path in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        rows += [r for r in csv.DictReader(open(path)) if "mmg::" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    for r in rows:
        name = re.sub(r"\(.*", "", r["Kernel_Name"]).replace("void ", "").replace("mmg::", "")
        dims = lambda stem: ",".join(r[stem + "_" + a] for a in "XYZ")
        print("%s grid %s wg %s lds %s" % (name, dims("Grid_Size"), dims("Workgroup_Size"), r["LDS_Block_Size"]))


if __name__ == "__main__":
    if len(sys.argv) < 3 or (sys.argv[1] != "--list" and (sys.argv[1] not in CASES or sys.argv[2] not in MODES + ("all",))):
        sys.exit(__doc__ + "\n\nCASE: %s\nMODE: %s | all" % (" | ".join(CASES), " | ".join(MODES)))
    if sys.argv[1] == "--list":
        listing(sys.argv[2])
        sys.exit(0)
    if "--lib" in sys.argv:
        from multimodalgame_amd import _lib
        _lib.LIB_PATH = os.path.join(REPO, "multimodalgame_amd", sys.argv[sys.argv.index("--lib") + 1])
    from multimodalgame_amd._lib import MmgError
    for m in (MODES if sys.argv[2] == "all" else (sys.argv[2],)):
        try:
            run(sys.argv[1], m)
        except MmgError as e:                  # a mode the case does not support: the library refused the call
            print("%s %s refused: %s" % (sys.argv[1], m, e))
