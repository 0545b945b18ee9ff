"""Float64 restatement of k_wgrad's job table (multimodalgame_amd/csrc/host_jobs.h: build_jobs) for the GPU tests of
tests/test_hip_wgrad.py.  Host only: numpy on arrays already fetched from the engine.

Every parameter block's gradient is one job
        out[n, k] = scale[n] * sum_{rows r} A[r, n] * Bm[r, k]
over one of four row sets: the (step, sample) rows r = t * B + b ("tb": only the LIVE ones count, t <= tstar[b], every row in
Fixed mode -- recomputed here from tstar, never from the kernel's own live-row list rmap / rcount), the B samples ("b"), the
D classes ("d") or the H sender units ("h", the code_bias job of the tile path).  A and Bm are the tape arrays k_wgrad reads
(or the virtual operand of the baselines, d score * linear2.weight * relu'(hidden)), taken from the engine's tape AFTER the
step; parameters a job reads (linear2.weight, code_layer.weight) are the ones the step STARTED from -- the fused step
updates them inside the same launch.

Besides the value, every job carries the sum of absolute products sum_r |A[r, n] Bm[r, k]| (what a rounding-error bound of
a sum scales with) and the per-row operands, so that a test can re-evaluate it with one row taken out or put in."""
import numpy as np

U32 = 2.0 ** -24            # unit roundoff of fp32

RECEIVER_ONLY_BINARY = ("w_h.weight", "w_h.bias", "w_d.weight", "w.weight", "w.bias", "s.weight", "s.bias")


# ---------------------------------------------------------------------------------------------- shape predicates
def dims_of(cfg):
    """Dims of an _lib.MmgConfig."""
    return dict(B=cfg.batch, T=cfg.max_exchange, H=cfg.h_dim, W=cfg.w_dim, R=cfg.rec_hidden, V=cfg.wv_dim,
                K=cfg.bas_hidden, D=cfg.n_classes, F=cfg.feat_dim, binary=bool(cfg.use_binary), fixed=bool(cfg.fixed_exchange))


def fast_shape(d):
    """host_select.h: fast_shape -- the register-resident kernels' agent shape (configs 1-3)."""
    return d["H"] == 256 and d["W"] == 32 and d["R"] == 64 and d["V"] == 100 and d["D"] <= 32 and d["T"] <= 16


def mc_shape(d):
    """layout.h: mc_shape -- the many-class register-resident conversation."""
    return d["H"] == 256 and d["W"] == 32 and d["R"] == 64 and d["V"] == 100 and 32 < d["D"] <= 1024 and d["T"] <= 16


def param_total(table):
    """layout.h: param_layout().total -- every tensor rounded up to 4 floats."""
    return max(e["offset"] + ((e["rows"] * max(e["cols"], 1) + 3) // 4) * 4 for e in table)


def wgrad_nsplit(TB, ptotal):
    """layout.h: wgrad_nsplit."""
    n = TB // 2048
    n = min(n, 16) if TB >= 4096 else 1
    cap = int(12000 // (ptotal // 512 + 64))
    return max(cap, 1) if n > cap else n


def wgrad_job_nsplit(TB, ptotal, job_tiles):
    """layout.h: wgrad_job_nsplit."""
    n = wgrad_nsplit(TB, ptotal)
    if TB > 2048 and job_tiles <= 64:
        n = max(n, min(TB // 320, 16))
    return n


# ---------------------------------------------------------------------------------------------- the job table
class Job(object):
    """One entry of build_jobs.  out: (agent, param name, r0, r1, c0, c1) -- the block of the parameter (1-D tensors viewed as
    [n, 1]) the job writes.  rows: "tb" | "b" | "d" | "h".  kind: "gemm" (MFMA tiles, may be row-split) | "col" (column sums)
    | "special" (the code_bias job of the register-resident path).  ops(env) -> (A [rows, N], Bm [rows, K], scale [N] or
    None, |Bm| to use in the absolute-product sum or None)."""

    def __init__(self, agent, name, region, rows, kind, ops, virt=False, bias=False):
        self.agent, self.name, self.region, self.rows, self.kind, self.ops = agent, name, region, rows, kind, ops
        self.virt, self.bias = virt, bias
        self.nsplit = 1
        self.label = "%s.%s[%d:%d, %d:%d]" % ((agent, name) + tuple(region))

    def shape(self):
        r0, r1, c0, c1 = self.region
        return (r1 - r0, c1 - c0)


def build_jobs(d, table, variant=None):
    """The jobs of build_jobs for dims `d` (dims_of) and the parameter table `table` (_lib.param_table), with the row-split
    plan (nsplit per GEMM job, bias columns as K = 1 GEMMs) k_wgrad takes.  variant: the code_bias job -- "fast" | "tile" |
    "generic" (host_jobs.h: the three CodeBiasJob branches of build_jobs; default: "fast" at fast_shape, else "tile")."""
    B, T, H, W, R, V, K, D = (d[k] for k in "BTHWRVKD")
    TB = T * B
    ent = {(e["agent"], e["name"]): e for e in table}
    ptotal = param_total(table)
    binary = d["binary"]
    if variant is None:
        variant = "fast" if fast_shape(d) else "tile"
    jobs = []

    def full(agent, name, c0=0, c1=None):
        e = ent[(agent, name)]
        return (0, e["rows"], c0, (max(e["cols"], 1) if c1 is None else c1))

    def tbv(name, lo=0):
        return lambda env: env["tb"](name, lo)

    def gemm(agent, name, rows, A, Bm, region=None, virt=False):
        jobs.append(Job(agent, name, region or full(agent, name), rows, "gemm", lambda env: (A(env), Bm(env), None, None), virt=virt))

    def col(agent, name, rows, src, scale=None, region=None, virt=False):
        jobs.append(Job(agent, name, region or full(agent, name), rows, "col",
                        lambda env: (src(env), np.ones((src(env).shape[0], 1)), scale(env) if scale else None, None), virt=virt))

    def wsum(agent, name, rows, wrow, src):               # dst[c] = sum_r wrow[r] src[r, c]  (out [1, cols])
        jobs.append(Job(agent, name, full(agent, name), rows, "col", lambda env: (wrow(env)[:, None], src(env), None, None)))

    def bias(agent, name, src):
        jobs.append(Job(agent, name, full(agent, name), "tb", "col",
                        lambda env: (src(env), np.ones((src(env).shape[0], 1)), None, None), bias=True))

    rec, sen, brc, bsn = "receiver", "sender", "baseline_rec", "baseline_sen"
    h_before, h_after = tbv("h", 0), tbv("h", 1)
    gemm(rec, "rnn.weight_ih", "tb", tbv("dgi"), tbv("z"))
    gemm(rec, "rnn.weight_hh", "tb", tbv("dgh"), h_before)
    bias(rec, "rnn.bias_ih", tbv("dgi"))
    bias(rec, "rnn.bias_hh", tbv("dgh"))
    gemm(rec, "y1.weight", "b", lambda env: env["t"]["dA"], lambda env: env["t"]["hstar"], region=full(rec, "y1.weight", 0, R))
    gemm(rec, "y1.weight", "d", lambda env: env["t"]["dC"], lambda env: env["t"]["descc"], region=full(rec, "y1.weight", R, R + V))
    col(rec, "y1.bias", "d", lambda env: env["t"]["dC"])
    wsum(rec, "y2.weight", "d", lambda env: np.ones(D), lambda env: env["t"]["Py2"])
    col(rec, "y2.bias", "b", lambda env: env["t"]["dysum"].reshape(B, 1))
    if binary:
        dls = lambda env: env["tb"]("dls")[:, 0]
        gemm(rec, "w_h.weight", "tb", tbv("dgpre"), h_after)
        bias(rec, "w_h.bias", tbv("dgpre"))
        gemm(rec, "w_d.weight", "tb", tbv("dgpre"), tbv("dbar"))
        gemm(rec, "w.weight", "tb", tbv("dlw"), tbv("g"))
        bias(rec, "w.bias", tbv("dlw"))
        wsum(rec, "s.weight", "tb", dls, h_after)
        col(rec, "s.bias", "tb", tbv("dls"))
        # ---- sender
        gemm(sen, "image_layer.weight", "b", lambda env: env["t"]["dhx"], lambda env: env["x"])
        col(sen, "image_layer.bias", "b", lambda env: env["t"]["dhx"])
        gemm(sen, "code_layer.weight", "tb", tbv("dpre"), tbv("c"))
        bias(sen, "code_layer.bias", tbv("dpre"))
        dsig = lambda env: env["t"]["dsig"]
        wc = lambda env: env["P"][sen]["code_layer.weight"]                     # [H, W], before the step
        if variant == "tile":       # dsig[j] * sum_h Wc[h, j] u0[h]   (u0 = sum_b dpre[0, b, :], formed by k_dhx)
            jobs.append(Job(sen, "code_bias", full(sen, "code_bias"), "h", "col",
                            lambda env: (wc(env), env["t"]["u0"].reshape(H, 1), dsig(env), None)))
        elif variant == "fast":     # ... with u0 formed inside k_wgrad from the step-0 rows of dpre
            def ops_fast(env):
                d0 = env["t"]["dpre"][0]                                         # [B, H]
                return wc(env), d0.sum(0).reshape(H, 1), dsig(env), np.abs(d0).sum(0).reshape(H, 1)
            jobs.append(Job(sen, "code_bias", full(sen, "code_bias"), "h", "special", ops_fast))
        else:                       # generic kernels: dc0 = W_c^T dpre_0 per sample
            col(sen, "code_bias", "b", lambda env: env["t"]["dc0"], scale=dsig)
        gemm(sen, "binary_layer.weight", "tb", tbv("dlz"), tbv("a"))
        bias(sen, "binary_layer.bias", tbv("dlz"))
        # ---- baselines: d hidden = d score * linear2.weight * relu'(hidden), never materialised
        for agent, beta, hid, inputs in ((brc, "dbr", "hid_r", (("z", W), ("h_after", R))),
                                         (bsn, "dbs", "hid_s", (("hx", H), ("zr", W)))):
            def vop(env, beta=beta, hid=hid, agent=agent):
                w2 = env["P"][agent]["linear2.weight"].reshape(-1)
                return env["tb"](beta)[:, :1] * w2[None, :] * (env["tb"](hid) > 0)
            c0 = 0
            for src, width in inputs:
                if src == "h_after":
                    op = h_after
                elif src == "hx":
                    op = lambda env: np.tile(env["t"]["hx"], (T, 1))            # row % B (magic-number division in k_wgrad)
                else:
                    op = tbv(src)
                gemm(agent, "linear1.weight", "tb", vop, op, region=full(agent, "linear1.weight", c0, c0 + width), virt=True)
                c0 += width
            col(agent, "linear1.bias", "tb", vop, virt=True)
            wsum(agent, "linear2.weight", "tb", (lambda env, beta=beta: env["tb"](beta)[:, 0]), tbv(hid))
            col(agent, "linear2.bias", "tb", tbv(beta))
    # ---- row-split plan (host_jobs.h: JobBuilder::gemm, bias_as_gemm, and plan_jobs' choice of wgrad_small_split)
    nrows = {"tb": TB, "b": B, "d": D, "h": H}

    def plan(small_split):
        as_gemm = wgrad_nsplit(TB, ptotal) > 1 or (small_split and TB > 2048)
        tiles, nblk = 0, 0
        for j in jobs:
            if j.bias:
                j.kind = "gemm" if as_gemm else "col"
            N, Kk = j.shape()
            if j.kind == "gemm":
                jt = ((N + 15) // 16) * ((Kk + 31) // 32)
                if nrows[j.rows] != TB:
                    j.nsplit = 1
                else:
                    j.nsplit = wgrad_job_nsplit(TB, ptotal, jt) if small_split else wgrad_nsplit(TB, ptotal)
                tiles += jt * j.nsplit
            else:
                j.nsplit = 1
                nblk += (N * Kk + 15) // 16 if j.kind == "col" else 1
        return tiles, tiles + nblk
    tiles, _ = plan(False)
    small = False
    if tiles <= 256 and TB > 2048:
        small = True
        _, nw = plan(True)
        if nw > 16384:
            small = False
            plan(False)
    for j in jobs:
        j.small_split = small
    return jobs


# ---------------------------------------------------------------------------------------------- evaluation
def live_rows(d, tstar):
    """[T * B] bool: row t * B + b is live (t <= tstar[b]; every row in Fixed mode)."""
    B, T = d["B"], d["T"]
    if d["fixed"]:
        return np.ones(T * B, bool)
    t = np.arange(T)[:, None]
    return (t <= np.asarray(tstar).reshape(1, B)).reshape(-1)


def make_env(d, tape, x, desc, params_before):
    """tape: {name: array} (float64 host copies of the engine's tape); params_before: {agent: {name: array}}."""
    B, T = d["B"], d["T"]
    t = {k: np.asarray(v, np.float64) for k, v in tape.items()}
    P = {a: {k: np.asarray(v, np.float64) for k, v in dd.items()} for a, dd in params_before.items()}

    def tb(name, lo=0):
        v = t[name]
        v = v[lo:lo + T] if name == "h" else v[:T]
        return v.reshape(T * B, -1)
    return dict(t=t, P=P, tb=tb, x=np.asarray(x, np.float64), desc=np.asarray(desc, np.float64))


def evaluate(job, env, live, extra_rows=None, drop_row=None):
    """(value [N, K], sum of |products| [N, K]) of one job.  live: [T * B] bool (row set "tb").  drop_row: a live row left
    out; extra_rows: (A rows, Bm rows) added (a dead row's stale operands)."""
    A, Bm, scale, Babs = job.ops(env)
    Bm_abs = np.abs(Bm) if Babs is None else Babs
    if job.rows == "tb":
        m = live.copy()
        if drop_row is not None:
            assert m[drop_row]
            m[drop_row] = False
        A, Bm, Bm_abs = A[m], Bm[m], Bm_abs[m]
    val = A.T @ Bm
    aps = np.abs(A).T @ Bm_abs
    if extra_rows is not None:
        ea, eb = extra_rows
        val = val + ea.T @ eb
        aps = aps + np.abs(ea).T @ np.abs(eb)
    if scale is not None:
        val = val * scale[:, None]
        aps = aps * np.abs(scale)[:, None]
    return val, aps


def n_chain(job, d, n_live):
    """Longest chain of dependent fp32 roundings k_wgrad applies to one output element of `job` (see
    tests/test_hip_wgrad.py for the derivation).  n_live: rows the job reduces over (live rows with the row list, T * B
    without it)."""
    rows = {"tb": n_live, "b": d["B"], "d": d["D"], "h": d["H"]}[job.rows]
    if job.kind == "gemm":
        chunks = -(-rows // 64)
        per_slice = -(-chunks // job.nsplit)
        return 16 * per_slice + 2 + job.nsplit + 1 + (1 if job.virt else 0)
    if job.kind == "special":
        return -(-d["B"] // 4) + 2 + max(32, d["H"] // 8) + 3 + 2
    return -(-rows // 64) + 64 + 12


def region_of(job, grads):
    """The block of the engine's gradient array (numpy, the parameter's shape) the job wrote, as [N, K] float64."""
    g = np.asarray(grads[job.agent][job.name], np.float64)
    g = g.reshape(g.shape[0], -1)
    r0, r1, c0, c1 = job.region
    return g[r0:r1, c0:c1]


def coverage(jobs, table, binary):
    """{(agent, name): int array of how many jobs write each float}."""
    cnt = {}
    for e in table:
        cnt[(e["agent"], e["name"])] = np.zeros((e["rows"], max(e["cols"], 1)), np.int64)
    for j in jobs:
        r0, r1, c0, c1 = j.region
        c = cnt[(j.agent, j.name)]
        assert j.shape() == (r1 - r0, c1 - c0) and r1 <= c.shape[0] and c1 <= c.shape[1], j.label
        c[r0:r1, c0:c1] += 1
    return cnt


# ---------------------------------------------------------------------------------------------- clip + optimizer
def clip_and_step(params, state, grads, agents, optim_type, lr, step, coef_rel_err=0.0):
    """float64 per-agent clip_grad_norm(max_norm = 1) + one torch.optim step (oracle/cpu_ref.py: build_optimizers,
    train_minibatch; torch.optim.RMSprop / Adam / SGD defaults).  params / grads: {agent: {name: array}}; state: {agent:
    {name: (s1, s2)}} (RMSprop square_avg | -, Adam exp_avg | exp_avg_sq).  Returns (new params, new state, norms)."""
    newp, news, norms = {}, {}, {}
    for a in agents:
        g = {k: np.asarray(v, np.float64) for k, v in grads[a].items()}
        norm = float(np.sqrt(sum(float((v * v).sum()) for v in g.values())))
        norms[a] = norm
        coef = min(1.0, 1.0 / (norm + 1e-6))
        newp[a], news[a] = {}, {}
        for k, gv in g.items():
            gv = gv * coef
            p = np.asarray(params[a][k], np.float64)
            s1, s2 = (np.asarray(s, np.float64) for s in state[a][k])
            if optim_type == "RMSprop":
                s1 = 0.99 * s1 + 0.01 * gv * gv
                p = p - lr * gv / (np.sqrt(s1) + 1e-8)
            elif optim_type == "Adam":
                s1 = 0.9 * s1 + 0.1 * gv
                s2 = 0.999 * s2 + 0.001 * gv * gv
                bc1, bc2 = 1 - 0.9 ** step, 1 - 0.999 ** step
                p = p - (lr / bc1) * s1 / (np.sqrt(s2) / np.sqrt(bc2) + 1e-8)
            else:
                p = p - lr * gv
            newp[a][k], news[a][k] = p, (s1, s2)
    return newp, news, norms
