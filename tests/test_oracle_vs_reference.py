"""Cross-check oracle == reference. The reference's side comes from tests/golden/reference_*.npz (recorded from the unmodified
reference by oracle/make_reference_fixtures.py); where the reference checkout is present it is also run live and must still
give what those fixtures hold."""
import json
import os

import numpy as np
import pytest
import torch

from oracle.make_reference_fixtures import LIVE_HW, LIVE_OPTS, live_image, tensor_digest
from oracle.ref_import import reference_available

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _fixture(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    return json.loads(bytes(z["meta"]).decode()), z


def _reference_outputs(name, hw_index):
    """the reference's output dict of live case (name, LIVE_HW[hw_index]): small tensors as stored, large ones as digests"""
    meta, z = _fixture("reference_live_outputs")
    (case,) = [c for c in meta["cases"] if c["config"] == name and c["image_hw"] == list(LIVE_HW[hw_index])]
    out = {}
    for k in case["keys"]:
        key = "%s/%d/%s" % (name, hw_index, k)
        out[k] = meta["digests"][key] if key in meta["digests"] else torch.from_numpy(z[key])
    return out


def _assert_equals_reference(got, want):
    assert set(got) == set(want)
    for k, w in want.items():
        if isinstance(w, dict):
            assert tensor_digest(got[k].numpy()) == w, k
        else:
            assert got[k].dtype == w.dtype and got[k].shape == w.shape, k
            assert torch.equal(got[k], w), k


@pytest.mark.parametrize("name,wseed", [("densepose_rcnn_R_50_FPN_s1x", 7), ("densepose_rcnn_R_50_FPN_s1x_legacy", 8),
                                        ("densepose_rcnn_R_101_FPN_DL_s1x", 9)])
def test_oracle_equals_reference_live(name, wseed):
    from densepose_torchscript_amd.config import get_config
    from densepose_torchscript_amd.weights import make_synthetic_state
    from oracle.ref_cpu import OracleModel
    cfg = get_config(name, LIVE_OPTS)
    state = make_synthetic_state(cfg, wseed)
    ref = None
    if reference_available():
        from oracle.ref_import import build_reference_predictor
        ref = build_reference_predictor(cfg, state)
    ora = OracleModel(cfg, state)
    for i, hw in enumerate(LIVE_HW):
        img = live_image(hw)
        want = _reference_outputs(name, i)
        if ref is not None:
            _assert_equals_reference(ref(img), want)
        _assert_equals_reference(ora(img), want)


def _reference_c2_conversion(cfg, blobs):
    """align_and_update_state_dicts(..., c2_conversion=True) of the reference on `blobs`, restricted to the model's keys"""
    meta, z = _fixture("reference_c2_conversion")
    assert meta["config"] == cfg.name
    theirs = {k: np.asarray(blobs[b]) for k, b in meta["blob_of"].items()}
    theirs.update({k: z[k] for k in z.files if k != "meta"})
    if reference_available():
        import logging
        from oracle.ref_import import _setup_path
        _setup_path()
        from detectron2.checkpoint.c2_model_loading import align_and_update_state_dicts
        from densepose_torchscript_amd.weights import param_shapes
        shapes = param_shapes(cfg)
        logging.disable(logging.CRITICAL)
        try:
            live = align_and_update_state_dicts({k: torch.empty(s) for k, s in shapes.items()},
                                                {k: torch.from_numpy(np.asarray(v)) for k, v in blobs.items()}, c2_conversion=True)
        finally:
            logging.disable(logging.NOTSET)
        live = {k: v.numpy() for k, v in live.items() if k in shapes}
        assert set(live) == set(theirs) and all(np.array_equal(live[k], theirs[k]) for k in live)
    return theirs


def test_caffe2_name_conversion_equals_reference():
    """c2_names.convert_caffe2_blobs == the reference's convert_c2_detectron_names + align_and_update_state_dicts
    (c2_model_loading.py:66-204, :207-299) on a Detectron1-style blob dict of the legacy R50 variant."""
    from densepose_torchscript_amd.c2_names import convert_caffe2_blobs
    from densepose_torchscript_amd.config import TINY_OPTS, get_config
    from densepose_torchscript_amd.weights import make_synthetic_state, param_shapes
    from test_c2_names import _to_caffe2_blobs
    cfg = get_config("densepose_rcnn_R_50_FPN_s1x_legacy", TINY_OPTS)
    state = make_synthetic_state(cfg, 31)
    blobs = {k: v for k, v in _to_caffe2_blobs(cfg, state).items() if not k.endswith("_momentum")}
    shapes = param_shapes(cfg)
    mine = convert_caffe2_blobs(blobs, shapes)
    theirs = _reference_c2_conversion(cfg, blobs)
    assert set(theirs) <= set(mine)
    assert {k for k in mine if k not in theirs} == {k for k in mine if k.endswith("running_mean") or k.endswith("running_var")}
    for k, v in theirs.items():
        assert np.array_equal(v, mine[k]), k


def _reference_state_dict(cfg, name, wseed, state):
    """the reference's DefaultPredictor.state_dict() for `state`, rebuilt from the recorded key structure"""
    meta, z = _fixture("reference_state_dicts")
    m = meta[name]
    assert m["weight_seed"] == wseed
    params = {c: torch.from_numpy(state[c].copy()) for c in set(m["alias"].values())}   # aliases share one tensor, as there
    sd = {k: torch.from_numpy(z["%s/%s" % (name, k)]) if k in m["extra"] else params[m["alias"][k]] for k in m["keys"]}
    if reference_available():
        from oracle.ref_import import build_reference_predictor
        live = build_reference_predictor(cfg, state).state_dict()
        assert list(live) == list(sd) and all(torch.equal(live[k], sd[k]) for k in sd)
    return sd


@pytest.mark.parametrize("name,wseed", [("densepose_rcnn_R_50_FPN_s1x", 17), ("densepose_rcnn_R_50_FPN_s1x_legacy", 18),
                                        ("densepose_rcnn_R_101_FPN_DL_s1x", 19)])
def test_load_checkpoint_reads_the_reference_state_dict(name, wseed, tmp_path):
    """weights.load_checkpoint on what the reference itself would save - `DefaultPredictor.state_dict()` as a torch `.pth`
    (bare and wrapped in {"model": ...}) and as a detectron2-style `.pkl` ({"model", "__author__"}, detection_checkpoint.py:53-64) -
    gives back the canonical state: the TorchScript fork's ModuleList aliases (stages.N / lateral_convs.N / ...) collapse onto
    the canonical names, the `model.` prefix, pixel_mean / pixel_std and the anchor buffers are dropped, values are untouched."""
    import pickle
    from densepose_torchscript_amd.config import TINY_OPTS, get_config
    from densepose_torchscript_amd.weights import check_state, load_checkpoint, make_synthetic_state, param_shapes
    cfg = get_config(name, TINY_OPTS)
    state = make_synthetic_state(cfg, wseed)
    sd = _reference_state_dict(cfg, name, wseed, state)
    assert len(sd) > len(state)                         # the aliases are really there
    shapes = param_shapes(cfg)
    pth, pth_wrapped, pkl = str(tmp_path / "m.pth"), str(tmp_path / "w.pth"), str(tmp_path / "m.pkl")
    torch.save(sd, pth)
    torch.save({"model": sd, "iteration": 7}, pth_wrapped)
    with open(pkl, "wb") as f:
        pickle.dump({"model": {k: v.numpy() for k, v in sd.items()}, "__author__": "reference state_dict"}, f, protocol=2)
    for path in (pth, pth_wrapped, pkl):
        got = load_checkpoint(path, cfg)
        assert check_state(cfg, got) == []              # nothing missing, nothing mis-shaped, nothing unknown
        assert set(got) == set(shapes) == set(state)
        for k in shapes:
            assert got[k].dtype == np.float32 and np.array_equal(got[k], state[k]), (path, k)
