#!/usr/bin/env python
"""The per-sample reverse pass (csrc/bwd_sample_parts.h) against the PARENT commit's library: same bits, same speed.

  bwd_ab.py --build [--parent REV] [--scratch DIR]   build REV's libmmg.so (default HEAD~1) in a `git worktree` under DIR and keep
                                                     it as DIR/libmmg_parent.so (needs git and hipcc, no GPU)
  bwd_ab.py [--scratch DIR]                          bit comparison, one training minibatch per case and library (below)
  bwd_ab.py --bench [--scratch DIR]                  speed: parent and tree alternating in one session, three runs each

Without --build an existing DIR/libmmg_parent.so is used as it is.  DIR defaults to $TMPDIR/mmg_bwd_ab.

Bit comparison: for each case one training minibatch from the same seed, weights and data with each library, in a fresh child
process each, one after the other, each under a time limit; the first non-zero exit ends the script.  Compared bit for bit: the
flat gradient buffer, the flat parameters after the update and the gradient tapes of the reverse pass on the live rows (steps
t <= t* of every sample).  Every kernel on these paths is deterministic (no float atomics), so the same expressions in the same
order give the same bits; exit code 1 on any difference.  Each case is the smallest the test suite uses that selects the kernel;
its launch plan (Engine.plan_text()) and the kernels it launched are printed.

Speed: bench.py (config 2: k_game_fast) and scripts/time_configs.py for c3 (k_bwd_conv_fast), c4 (k_bwd_sample) and c5 (k_bwd_mc2).
A line passes when the tree's median lies inside the parent's own min-max spread of the session or on the better side of it."""
import argparse, json, os, re, shutil, statistics, subprocess, sys, tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
TREE_LIB = os.path.join(REPO, "multimodalgame_amd", "libmmg.so")
TAPES = ("dgi", "dgh", "dlw", "dlz", "dgpre", "dpre", "dhx", "dls", "dbs", "dbr", "dy", "dA", "Astar", "hstar", "dysum")
CONTINUOUS = dict(use_binary=False, fixed_exchange=True, max_exchange=4, entropy_s=None, entropy_sen=None, entropy_rec=None)
CASES = {   # name: (engine kwargs over bench.C2 -- config 1's agents --, batch, environment, phased)
    "k_game_fast: fused Adaptive step, D = 30, T = 10": (dict(), 16, {}, False),
    "k_bwd_conv_fast<MERGED, MERGE_DC>: the same under MMG_NO_GAME=1": (dict(), 16, {"MMG_NO_GAME": "1"}, False),
    "k_bwd_conv_fast<no MERGED>: the phased step of the same": (dict(), 16, {}, True),
    "k_bwd_sample: H = 128, W = 64, T = 5": (dict(h_dim=128, w_dim=64, max_exchange=5), 16, {}, False),
    "k_bwd_mc2: continuous messages, D = 100 (the kernel kept its own copy: the same code on both sides)": (dict(CONTINUOUS, n_classes=100), 16, {}, False),
}
BENCH = (("bench.py (config 2: k_game_fast)", None, True), ("time_configs.py c3 (k_bwd_conv_fast)", "c3", False),
         ("time_configs.py c4 (k_bwd_sample)", "c4 W", False), ("time_configs.py c5 (k_bwd_mc2)", "c5", False))


def child(name, lib, out):
    import numpy as np, torch
    from multimodalgame_amd import _lib
    _lib.LIB_PATH = lib
    import bench
    from multimodalgame_amd.engine import Engine
    from multimodalgame_amd.agents import init_state_dicts
    kw, B, _, phased = CASES[name]
    cfg = dict(bench.C2); cfg.update(kw)
    eng = Engine(batch=B, **cfg)
    eng.load_state_dicts(init_state_dicts(eng, seed=0))
    feats, target, desc = bench.synthetic_dataset(max(3000, B), cfg["n_classes"], cfg["feat_dim"], cfg["wv_dim"])
    x, t, d = (torch.from_numpy(a).to(eng.device) for a in (feats[:B], target[:B], desc))
    # the launch list, printed with the plan: profiling only brackets every launch with two events on its stream (host_launch.h:
    # Scope); kernel selection, the fused step and the launch order do not look at the flag
    eng.set_profiling(True)
    launches = []
    for call in ((lambda: eng.forward(x, t, d, seed=11, train=True), eng.loss_stats, lambda: eng.backward(x, t, d), eng.clip_step) if phased
                 else (lambda: eng.train_step(x, t, d, seed=11),)):
        call()
        torch.cuda.synchronize()
        launches += [n for n, _ in eng.kernel_times()]
    eng.check_sync()
    T, tstar = cfg["max_exchange"], eng.tape["tstar"][:B].cpu().numpy().astype(np.int64)
    arrays = {"grads": eng.flat_grads.cpu().numpy(), "params": eng.flat_params.cpu().numpy(), "tstar": tstar}
    for k in TAPES:
        a = eng.tape[k].cpu().numpy()
        if tuple(a.shape[:2]) == (T, B):                                 # [T, B, ...]: the live rows (dead ones zeroed); the others are [B, ...]
            a = a.copy()
            a[np.arange(T)[:, None] > tstar[None, :]] = 0
        arrays["tape_" + k] = a
    np.savez(out, **arrays)
    print("PLAN " + json.dumps(eng.plan_text() + "launches: " + " ".join(launches)))


def run_child(name, lib, out, env):
    p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "--child", name, "--lib", lib, "--out", out],
                       env=dict(os.environ, **env), capture_output=True, text=True)
    if p.returncode != 0:
        print("   child exited with %d (%s):\n%s" % (p.returncode, lib, p.stderr[-2000:]))
        sys.exit(2)
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("PLAN ")][0][5:])


def compare(parent_lib):
    import numpy as np
    bad = 0
    print("# launches: the library's timer scopes, one per launch group (mmg.hip).  k_game = k_game_fast; k_bwd_conv in family 0 =\n"
          "# k_bwd_conv_fast (MERGED in the fused step, not in the phased one); k_bwd_tile with `receiver 0 (0 sample ...)` in the plan =\n"
          "# k_bwd_pre + k_bwd_sample; k_bwd_mc = k_bwd_mc1 + k_bwd_mc2")
    with tempfile.TemporaryDirectory() as tmp:
        for name, (kw, B, env, phased) in CASES.items():
            print(name)
            plans = [run_child(name, lib, os.path.join(tmp, tag + ".npz"), env) for tag, lib in (("parent", parent_lib), ("tree", TREE_LIB))]
            print("   plan: " + plans[1].strip().replace("\n", "\n         "))
            if plans[0] != plans[1]:
                print("   the parent's plan differs: " + plans[0]); bad += 1
            a, b = np.load(os.path.join(tmp, "parent.npz")), np.load(os.path.join(tmp, "tree.npz"))
            same, diff = [], []
            for k in a.files:
                va, vb = a[k].reshape(-1), b[k].reshape(-1)
                n = int((va.view(np.uint32 if va.dtype == np.float32 else va.dtype) != vb.view(np.uint32 if vb.dtype == np.float32 else vb.dtype)).sum())
                (diff if n else same).append("%s (%d of %d)" % (k, n, va.size) if n else k)
            print("   live steps %d of %d, nonzero gradients %d" % (int((a["tstar"] + 1).sum()), B * len(a["tape_dls"]), int((a["grads"] != 0).sum())))
            print("   bit-identical: " + " ".join(same))
            if diff:
                print("   DIFFERENT: " + " ".join(diff)); bad += 1
    print("OK: every array bit-identical in every case" if not bad else "MISMATCH in %d case(s)" % bad)
    return 1 if bad else 0


def bench_once(lib, prefix):
    if prefix is None:
        code = "import sys; sys.path.insert(0, %r); from multimodalgame_amd import _lib; _lib.LIB_PATH = %r; import bench; sys.argv = ['bench.py']; bench.main()" % (REPO, lib)
    else:
        code = ("import sys, runpy; sys.path.insert(0, %r); from multimodalgame_amd import _lib; _lib.LIB_PATH = %r; sys.argv = ['time_configs.py', %r]; "
                "runpy.run_path(%r, run_name='__main__')" % (REPO, lib, prefix, os.path.join(REPO, "scripts", "time_configs.py")))
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", code], capture_output=True, text=True, cwd=REPO)
    if p.returncode != 0:
        print("   run exited with %d (%s):\n%s" % (p.returncode, lib, p.stderr[-2000:]))
        sys.exit(2)
    if prefix is None:
        return float(json.loads(p.stdout.strip().splitlines()[-1])["value"])
    return float(re.search(r"([\d.]+) us/minibatch", [l for l in p.stdout.splitlines() if l.startswith(prefix)][0]).group(1))


def bench_ab(parent_lib):
    ok = True
    for title, prefix, higher_better in BENCH:
        unit = "exchange steps/s (higher is better)" if higher_better else "us/minibatch (lower is better)"
        vals = {"parent": [], "tree": []}
        for run in range(3):
            for tag, lib in (("parent", parent_lib), ("tree", TREE_LIB)):
                vals[tag].append(bench_once(lib, prefix))
                print("%s %s run %d %s" % (title, tag, run + 1, vals[tag][-1]), flush=True)
        lo, hi = min(vals["parent"]), max(vals["parent"])
        mp, mt = statistics.median(vals["parent"]), statistics.median(vals["tree"])
        good = (mt >= lo) if higher_better else (mt <= hi)
        ok = ok and good
        print("%s: %s\n   parent %s median %s min-max %s .. %s\n   tree   %s median %s   %s" % (
            title, unit, vals["parent"], mp, lo, hi, vals["tree"], mt, "PASS" if good else "FAIL"), flush=True)
    return 0 if ok else 1


def build_parent(rev, scratch):
    wt = os.path.join(scratch, "parent")
    if os.path.exists(wt):
        subprocess.check_call(["git", "worktree", "remove", "--force", wt], cwd=REPO)
    subprocess.check_call(["git", "worktree", "add", "--detach", wt, rev], cwd=REPO)
    subprocess.check_call([sys.executable, "-c", "from multimodalgame_amd import build; build.build_library(force=True)"], cwd=wt)
    shutil.copy(os.path.join(wt, "multimodalgame_amd", "libmmg.so"), os.path.join(scratch, "libmmg_parent.so"))
    sha = subprocess.check_output(["git", "rev-parse", "--short", rev], cwd=REPO, text=True).strip()
    open(os.path.join(scratch, "parent_rev"), "w").write(sha + "\n")
    subprocess.check_call(["git", "worktree", "remove", "--force", wt], cwd=REPO)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true"); ap.add_argument("--bench", action="store_true")
    ap.add_argument("--parent", default="HEAD~1"); ap.add_argument("--scratch", default=os.path.join(tempfile.gettempdir(), "mmg_bwd_ab"))
    ap.add_argument("--child"); ap.add_argument("--lib"); ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.lib, a.out)
        sys.exit(0)
    scratch = os.path.abspath(a.scratch)
    os.makedirs(scratch, exist_ok=True)
    if a.build:
        build_parent(a.parent, scratch)
        sys.exit(0)
    parent_lib = os.path.join(scratch, "libmmg_parent.so")
    if not os.path.exists(parent_lib):
        sys.exit("no %s: run `bwd_ab.py --build` where git and hipcc are" % parent_lib)
    print("# parent commit %s against the tree, %s" % (open(os.path.join(scratch, "parent_rev")).read().strip(), "speed" if a.bench else "bit comparison"))
    sys.exit(bench_ab(parent_lib) if a.bench else compare(parent_lib))
