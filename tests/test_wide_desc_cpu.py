"""Wide class descriptions (-wv_dim 200 / 300 / up to 512) without a GPU: the CPU oracle against the g10 fixtures (the
reference's own run at V = 300 and at V = 50, tests/golden/make_golden_wide.py), the layout queries of the C-ABI at the new
limit, and the description pipeline on a 300-d GloVe file."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from multimodalgame_amd import _lib
from multimodalgame_amd.misc import write_synthetic_dataset
from multimodalgame_amd.model import _desc_matrix
from tests import common
from tests.test_oracle_golden import _oracle_train_case_portable

WIDE_CASES = ["g10_wide_desc_adaptive", "g10_wide_desc_fixed", "g10_wide_desc_continuous", "g10_wide_desc_tiny50"]
G2_BYTES = os.path.getsize(os.path.join(common.GOLDEN_DIR, "g2_adaptive_c1.npz"))


@pytest.mark.parametrize("name", WIDE_CASES)
def test_oracle_matches_reference_at_wide_v(name, tmp_path):
    """The oracle (oracle/cpu_ref.py, unchanged) against the reference's own run, tolerances of tests/test_oracle_golden.py."""
    z, meta = common.load_golden(name)
    assert meta["wv_dim"] == (50 if name.endswith("tiny50") else 300)
    got = _oracle_train_case_portable(name, str(tmp_path / "oracle.npz"))
    problems = common.compare_packed(got, z, atol=2e-6, rtol=2e-5, ulps=1)
    assert not problems, "\n".join(problems[:20])


@pytest.mark.parametrize("name", WIDE_CASES)
def test_fixture_is_small_and_holds_outputs_only(name):
    path = os.path.join(common.GOLDEN_DIR, name + ".npz")
    assert os.path.getsize(path) < G2_BYTES // 2
    z, meta = common.load_golden(name)
    assert not any(k.endswith((".x", ".desc")) for k in z.files)          # inputs by seed (common.case_inputs)
    _, _, desc, _ = common.case_inputs(meta, 0, name)
    assert desc.shape == (meta["n_classes"], meta["wv_dim"])


def test_adaptive_fixture_has_dead_rows():
    z, meta = common.load_golden("g10_wide_desc_adaptive")
    masks = z["mb0.s_masks"][:, :, 0]
    assert 0 < masks[1].sum() < masks.shape[1], "stop bits should be mixed at step 0"


def _cfg(V, **kw):
    d = dict(batch=64, n_classes=30, feat_dim=512, h_dim=256, w_dim=32, rec_hidden=64, wv_dim=V, bas_hidden=500, max_exchange=10,
             fixed_exchange=False)
    d.update(kw)
    return _lib.make_config(**d)


@pytest.mark.parametrize("V", [50, 200, 300, 512])
def test_layout_queries_accept_wide_v(V):
    lib = _lib.load()
    cfg = _cfg(V)
    n = lib.mmg_param_count(C.byref(cfg))
    assert n > 0, lib.mmg_last_error()
    table = {e["name"]: e for e in _lib.param_table(cfg) if e["agent"] == "receiver"}
    assert lib.mmg_workspace_bytes(C.byref(cfg)) > 0
    assert lib.mmg_grad_floats(C.byref(cfg)) > n
    assert lib.mmg_tape_table(C.byref(cfg), None, 0) > 0
    assert (table["y1.weight"]["rows"], table["y1.weight"]["cols"]) == (64, 64 + V)
    assert (table["w_d.weight"]["rows"], table["w_d.weight"]["cols"]) == (64, V)


def test_layout_queries_refuse_beyond_the_cap():
    lib = _lib.load()
    for V in (513, 516, 1024):
        cfg = _cfg(V)
        assert lib.mmg_param_count(C.byref(cfg)) < 0
        msg = lib.mmg_last_error().decode()
        assert "wv_dim" in msg and "512" in msg, msg
        assert lib.mmg_workspace_bytes(C.byref(cfg)) < 0
        assert lib.mmg_tape_table(C.byref(cfg), None, 0) < 0


def test_param_count_grows_with_v_as_the_two_description_matrices():
    lib = _lib.load()
    n100, n300 = (lib.mmg_param_count(C.byref(_cfg(V))) for V in (100, 300))
    assert n300 - n100 == 2 * 64 * 200              # y1.weight[:, R:] and w_d.weight, R = 64 rows each


def test_synthetic_data_and_glove_reader_round_trip_300d(tmp_path):
    """-synthetic_data writes a 300-d GloVe-format file; the description pipeline (read_data, embed, cbow) turns it into the
    [D, 300] matrix whose rows are the means of the four word vectors the file holds for each class."""
    paths = write_synthetic_dataset(str(tmp_path / "syn"), n_classes=7, per_class=3, feat_dim=16, wv_dim=300)
    assert paths["glove_path"].endswith("glove.synthetic.300d.txt")
    rows = {}
    with open(paths["glove_path"]) as f:
        for line in f:
            head, *vals = line.split()
            rows[head] = np.array(vals, dtype=np.float32)
            assert len(vals) == 300
    desc, map_labels = _desc_matrix(paths["descr_train"], paths["glove_path"], 300)
    assert tuple(desc.shape) == (7, 300) and desc.dtype == torch.float32
    for c in range(7):
        want = np.stack([rows["w%dx%d" % (c, j)] for j in range(4)]).sum(0) / 4.0
        np.testing.assert_allclose(desc[map_labels(c)].numpy(), want, rtol=1e-6, atol=1e-7)
