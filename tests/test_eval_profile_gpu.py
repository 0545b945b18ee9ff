"""mmg_eval_steps_profile on the GPU (include/mmg.h; csrc/kernels_eval.h: k_eval_profile).  Every case runs
Engine.eval_steps(..., prof=...), clones the tape behind the call and requires EXACT integer equality of every block with the
numpy restatement (tests/eval_profile_ref.py: np_eval_profile) on that tape -- the GPU's own floats with strict >, so there is no
tolerance and no excluded sample -- and, in the same call, acc / lens / batch equal to a plain eval_steps run of the same engine.
Three cases are also compared with the CPU oracle's own conversation (steps, rank, class_hits): tests/test_eval_profile_cpu.py
shows that their logits and stop probabilities are far from every tie.  Shapes and seeds: tests/test_eval_steps_cpu.py (CASES)
and tiny_W70 (tests/eval_profile_ref.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from multimodalgame_amd import _lib, commstats
from multimodalgame_amd.game import EvalAccumulator
from oracle import cpu_ref
from tests import common
from tests import eval_profile_ref as ref

pytestmark = pytest.mark.gpu

GPU_CASES = ["tiny_ragged", "tiny_all_stop", "tiny_never_stop", "tiny_T1", "tiny_fixed", "tiny_topk_ge_D", "tiny_continuous",
             "c1_B64", "D130_B17", "D1000_B16", "tiny_W70"]
ORACLE_CASES = ("tiny_ragged", "tiny_never_stop", "tiny_W70")


def _engine(meta, s_bias=None, batch=None):
    eng = common.make_engine(meta, **({} if batch is None else dict(batch=batch)))
    if s_bias is not None:
        eng.params["receiver"]["s.bias"].fill_(float(s_bias))
    return eng


def _tape(eng):
    """Clones of the tape arrays the profile reads, enqueued right behind the call."""
    tp, B, T = eng.tape, eng.cfg.batch, eng.cfg.max_exchange
    return dict(mask=tp["mask"].view(T + 1, B).clone(), s=tp["s"].view(T, B).clone(), z=tp["z"].view(T, B, -1).clone(),
                w=tp["w"].view(T, B, -1).clone(), y=tp["y"].view(T, B, -1).clone())


def _host(tape):
    return {k: v.cpu().numpy() for k, v in tape.items()}


def _dev(eng, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(eng.device) for a in arrays]


def _parse(eng, prof):
    return ref.parse(prof.cpu().numpy(), eng.cfg.n_classes, eng.cfg.max_exchange, eng.cfg.w_dim)


def _profiled(eng, xd, td, dd, top_k, mask=None):
    """One profiled call on a zeroed accumulator pair -> (parsed profile, acc, lens, batch rows, host tape)."""
    acc, prof = eng.eval_acc(), eng.eval_profile()
    lens, rows = eng.eval_steps(xd, td, dd, 1, top_k, acc, prof=prof, corrupt_mask=mask)
    tape = _tape(eng)
    torch.cuda.synchronize()
    eng.check_sync()
    return _parse(eng, prof), acc.cpu().numpy(), lens.cpu().numpy(), rows.cpu().numpy(), _host(tape)


@pytest.mark.parametrize("name", GPU_CASES)
def test_profile_equals_the_restatement_on_the_gpu_tape(name):
    c, meta, x, target, desc = ref.case_inputs(name)
    D, T, k = c["n_classes"], meta["max_exchange"], c["top_k"]
    fixed, binary = meta["fixed_exchange"], bool(meta["use_binary"])
    eng = _engine(meta, c["s_bias"])
    xd, td, dd = _dev(eng, x, target, desc)
    acc0 = eng.eval_acc()
    lens0, rows0 = eng.eval_steps(xd, td, dd, 1, k, acc0)                       # the plain entry: the old results do not move
    got, acc, lens, rows, tape = _profiled(eng, xd, td, dd, k)
    np.testing.assert_array_equal(acc, acc0.cpu().numpy())
    np.testing.assert_array_equal(lens, lens0.cpu().numpy())
    np.testing.assert_array_equal(rows, rows0.cpu().numpy())
    want = ref.np_eval_profile(tape, target, k, fixed, binary)
    print(name, "steps", got["steps"].sum(0).tolist(), "rank[T-1][:8]", got["rank"][T - 1][:8].tolist(), "hits", int(acc[0]),
          "bits", int(got["msg_sen"].sum()), int(got["msg_rec"].sum()))
    ref.assert_profile_equal(got, want, name)
    assert got["head"].tolist() == [1, c["batch"], 0, 0]
    assert got["rank"][T - 1, :min(k, D)].sum() == acc[0] == got["class_hits"].sum()
    if binary:
        assert got["msg_sen"][0].sum() > 0 and got["msg_rec"][0].sum() > 0
    else:
        assert not got["msg_sen"].any() and not got["msg_rec"].any()
    again = _profiled(eng, xd, td, dd, k)[0]                                     # the same call into a second zeroed accumulator
    ref.assert_profile_equal(again, got, name + " (second call)")
    if name in ORACLE_CASES:                                                     # ... and the CPU oracle's own conversation
        oc, ometa, otarget, otape = ref.oracle_case(name)
        op = ref.np_eval_profile(otape, otarget, k, fixed, binary)
        for blk in ("steps", "rank", "class_hits"):
            np.testing.assert_array_equal(got[blk], op[blk], err_msg="%s against the oracle: %s" % (name, blk))


def test_two_batch_sizes_share_one_accumulator():
    """Engines of batch 5 and 3 (the short final dev batch) add to ONE profile through EvalAccumulator(profile=True)."""
    c, meta, x, target, desc = ref.case_inputs("tiny_ragged")
    D, T, W = c["n_classes"], meta["max_exchange"], meta["rec_w_dim"]
    x1, target1, _ = cpu_ref.synthetic_batch(3, D, meta["img_feat_dim"], meta["wv_dim"], seed=c["seed_data"] + 1)
    acc = EvalAccumulator(D, c["top_k"], profile=True)
    wants = []
    for xb, tb in ((x, target), (x1, target1)):
        eng = _engine(meta, c["s_bias"], batch=len(xb))
        xd, td, dd = _dev(eng, xb, tb, desc)
        acc.add(eng, xd, td, dd, 1)
        wants.append((_tape(eng), tb))
    torch.cuda.synchronize()
    got = acc.fetch()
    want = ref.add_profiles([ref.np_eval_profile(_host(tp), tb, c["top_k"], False) for tp, tb in wants])
    ref.assert_profile_equal(got["profile"], want, "shared accumulator")
    ref.assert_profile_equal(ref.parse(acc.prof.cpu().numpy(), D, T, W), want, "shared accumulator, the tests' parser")
    assert got["profile"]["head"].tolist() == [2, 8, 0, 0] and got["samples"] == 8 and got["batches"] == 2
    assert got["profile"]["rank"][T - 1, :c["top_k"]].sum() == got["hits"]
    plain = EvalAccumulator(D, c["top_k"])                                       # profile=False: the keys of fetch() are the old ones
    assert "profile" not in plain.fetch() and sorted(set(got) - {"profile"}) == sorted(plain.fetch())


def test_targets_outside_the_classes_count_in_the_head_only():
    c, meta, x, target, desc = ref.case_inputs("tiny_ragged")
    D, k = c["n_classes"], c["top_k"]
    bad = target.copy()
    bad[1], bad[3] = D, -1
    eng = _engine(meta, c["s_bias"])
    xd, td, dd = _dev(eng, x, bad, desc)
    got, acc, _, _, tape = _profiled(eng, xd, td, dd, k)
    assert got["head"].tolist() == [1, 3, 2, 0]
    keep = np.array([0, 2, 4])
    sub = dict(mask=tape["mask"][:, keep], s=tape["s"][:, keep], z=tape["z"][:, keep], w=tape["w"][:, keep], y=tape["y"][:, keep])
    # (a sample's output step does not depend on the other samples: the masks are a running minimum, so every mask of a sample
    #  behind the batch's last executed step is 0 anyway)
    without = ref.np_eval_profile(sub, target[keep], k, False)
    for blk, _ in ref.BLOCKS:
        np.testing.assert_array_equal(got[blk], without[blk], err_msg=blk)
    ref.assert_profile_equal(got, ref.np_eval_profile(tape, bad, k, False), "restatement with the two targets")
    assert got["steps"].sum() == 3 and got["rank"].sum(1).tolist() == [3] * meta["max_exchange"]


def test_corruption_mask_is_counted_as_the_receiver_saw_it():
    c, meta, x, target, desc = ref.case_inputs("tiny_ragged")
    eng = _engine(meta, c["s_bias"])
    xd, td, dd = _dev(eng, x, target, desc)
    clean = _profiled(eng, xd, td, dd, c["top_k"])[0]
    mask = torch.tensor([1, 0, 0, 1, 0, 1], dtype=torch.float32).view(-1, 1)
    got, _, _, _, tape = _profiled(eng, xd, td, dd, c["top_k"], mask=mask)
    ref.assert_profile_equal(got, ref.np_eval_profile(tape, target, c["top_k"], False), "corrupted")
    assert not np.array_equal(got["msg_sen"], clean["msg_sen"]), "the mask should change the sender's bits that are counted"


def test_null_profile_is_an_error_that_names_the_plain_entry():
    c, meta, x, target, desc = ref.case_inputs("tiny_ragged")
    eng = _engine(meta, c["s_bias"])
    xd, td, dd = _dev(eng, x, target, desc)
    acc = eng.eval_acc()
    lens, rows = eng.eval_steps(xd, td, dd, 1, 2, acc)
    p = lambda t: C.c_void_p(t.data_ptr())
    before = acc.clone()
    args = [eng.handle, p(xd), p(td), 1, p(dd), 2, p(acc), p(lens), p(rows), None, eng._stream()]
    assert eng.lib.mmg_eval_steps_profile(*args) < 0
    assert b"mmg_eval_steps " in eng.lib.mmg_last_error() and b"prof" in eng.lib.mmg_last_error()
    prof = eng.eval_profile()
    args[9] = p(prof)
    for i in (0, 1, 2, 4, 6, 7, 8):                                              # what mmg_eval_steps refuses
        a = list(args)
        a[i] = None
        assert eng.lib.mmg_eval_steps_profile(*a) < 0, i
    torch.cuda.synchronize()
    assert torch.equal(acc, before) and not prof.any(), "a refused call enqueues nothing"
    assert int(eng.tape["counter"][0]) == 0


def test_profile_kernel_runs_under_the_new_entry_only():
    c, meta, x, target, desc = ref.case_inputs("c1_B64")
    eng = _engine(meta, c["s_bias"])
    xd, td, dd = _dev(eng, x, target, desc)

    def names(n, **kw):
        eng.set_profiling(True)
        eng.eval_steps(torch.cat([xd] * n), torch.cat([td] * n), dd, n, c["top_k"], eng.eval_acc(), **kw)
        torch.cuda.synchronize()
        out = [name for name, _ in eng.kernel_times()]
        eng.set_profiling(False)
        return out
    plain = names(1)
    assert "k_eval_profile" not in plain and plain[-1] == "k_eval_reduce", plain
    prof = eng.eval_profile()
    both = names(2, prof=prof)
    assert both == (plain + ["k_eval_profile"]) * 2, (plain, both)              # one launch per batch, directly behind k_eval_reduce
    assert int(prof[0]) == 2 and int(prof[1]) == 2 * c["batch"]
    assert int(eng.tape["counter"][0]) == 0                                      # the minibatch counter is untouched


def test_visual_attention_handle():
    from tests import test_visual_attn_gpu as vg, visual_attn_ref as vref
    m = vref.meta("B")
    eng = vg._engine(m)
    (xd, td, dd), _, g = vg._inputs(m, eng)
    eng.set_data_context(g)
    got, acc, _, _, tape = _profiled(eng, xd, td, dd, 2)
    fixed = bool(common.flags_from_meta(m).fixed_exchange)
    ref.assert_profile_equal(got, ref.np_eval_profile(tape, td.cpu().numpy(), 2, fixed), "visual attention")
    assert got["head"][1] == eng.cfg.batch and got["rank"][-1, :2].sum() == acc[0]


def test_description_attention_handle():
    from tests import desc_attn_ref as dref, test_desc_attn_gpu as dg
    m = dref.meta("B", seed_data=dref.EVAL_DATA_SEED["B"])
    eng = dg._engine(m)
    (xd, td, dd), _ = dg._inputs(m, eng)
    got, acc, _, _, tape = _profiled(eng, xd, td, dd, 2)
    fixed = bool(common.flags_from_meta(m).fixed_exchange)
    ref.assert_profile_equal(got, ref.np_eval_profile(tape, td.cpu().numpy(), 2, fixed), "description attention")
    assert got["head"][1] == eng.cfg.batch and got["rank"][-1, :2].sum() == acc[0]


def test_eval_dev_profile_library_form_equals_torch_form(tmp_path, monkeypatch):
    """model.eval_dev(profile=...) on the HIP engine over two dev batches, the second one short: the library form (one
    k_eval_profile launch per batch) equals the torch form on the same engine (MMG_EVAL_TORCH=1), and nothing else moves."""
    from multimodalgame_amd import flags as _flags
    from multimodalgame_amd.engine import Engine
    try:
        game, run, batches, desc, meta, z = ref.g8_game(tmp_path, "cuda:0", monkeypatch)
        calls = []
        real = Engine.eval_steps
        monkeypatch.setattr(Engine, "eval_steps", lambda self, *a, **kw: (calls.append("prof" in kw), real(self, *a, **kw))[1])
        lib_prof, py_prof = {}, {}
        acc_plain, extra_plain = run("plain.txt")
        acc_lib, extra_lib = run("lib.txt", profile=lib_prof)
        assert calls == [False, False, True, True], calls
        monkeypatch.setenv("MMG_EVAL_TORCH", "1")
        acc_py, extra_py = run("py.txt", profile=py_prof)
        assert len(calls) == 4, "MMG_EVAL_TORCH=1 is the torch form"
        assert acc_lib == acc_plain and extra_lib == extra_plain and acc_lib == pytest.approx(acc_py, abs=1e-12)
        assert open(str(tmp_path / "lib.txt")).read() == open(str(tmp_path / "plain.txt")).read() == open(str(tmp_path / "py.txt")).read()
        ref.assert_profile_equal(lib_prof, py_prof, "eval_dev: library form against torch form")
        n = sum(len(x) for x, _ in batches)
        assert lib_prof["head"].tolist() == [2, n, 0, 0] and lib_prof["steps"].sum() == n
        s = commstats.summarise(lib_prof, 2)
        assert s["acc_by_step"][-1] * n == pytest.approx(acc_lib * 2 * int(z["batch"]), abs=1e-9)    # (eval_dev: nominal batch size in the denominator)
    finally:
        _flags.FLAGS.Reset()
