"""Pins the product's config mapping to the reference's own config tree.

oracle/ref_import.py builds the reference FROM the product's ModelConfig when goldens are made, so a wrong default in
config.py would poison golden and product alike. Here the direction is reversed: the reference's
get_cfg() + add_densepose_config + merge_from_file(yaml) (export.py:22-34, + SCORE_THRESH_TEST from export.py:15,23-24)
is the source, and every key the product maps or hard-wires must agree with it for all five BASELINE configs. The reference's
effective values are tests/golden/reference_configs.json (recorded by oracle/make_reference_fixtures.py); where the reference
checkout is present they are also read live and must still be what that file holds."""
import json
import os

import pytest
import yaml

from oracle.make_reference_fixtures import CONFIGS
from oracle.ref_import import REFERENCE_ROOT, reference_available

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_configs.json")


def _reference_values(name):
    """dotted key -> the reference's effective value (lists for sequences) of every key config.py maps or hard-wires"""
    with open(FIXTURE) as f:
        vals = json.load(f)[name]
    if reference_available():
        from oracle.make_reference_fixtures import _get, _plain, reference_cfg
        from densepose_torchscript_amd.config import _FIXED_KEYS, _KEYMAP
        ref = reference_cfg(name)
        live = {}
        for key in list(_KEYMAP) + list(_FIXED_KEYS):
            v, present = _get(ref, key)
            if present:
                live[key] = _plain(v)
        assert live == vals, "tests/golden/reference_configs.json is stale: python -m oracle.make_reference_fixtures"
    return vals


def _write_yaml_pair(directory, name, vals):
    """the recorded values as a two-file yaml config (<name>.yaml with _BASE_: Base.yaml), half of the keys in each file"""
    trees = ({}, {"_BASE_": "Base.yaml"})
    for i, (key, v) in enumerate(sorted(vals.items())):
        node = trees[i % 2]
        *parents, leaf = key.split(".")
        for p in parents:
            node = node.setdefault(p, {})
        node[leaf] = v
    for fn, tree in zip(("Base.yaml", name + ".yaml"), trees):
        with open(os.path.join(directory, fn), "w") as f:
            yaml.safe_dump(tree, f)
    return os.path.join(directory, name + ".yaml")


@pytest.mark.parametrize("name", CONFIGS)
def test_every_mapped_key_equals_the_reference(name, tmp_path):
    from densepose_torchscript_amd.config import _KEYMAP, get_config
    ref, mine = _reference_values(name), get_config(name)
    checked = 0
    for key, (field, conv) in _KEYMAP.items():
        assert key in ref, "reference has no key %s" % key
        assert getattr(mine, field) == conv(ref[key]), (name, key, getattr(mine, field), ref[key])
        checked += 1
    assert checked == len(_KEYMAP) >= 30
    # the same holds when the product reads a yaml itself (with _BASE_ inheritance): the reference's own yaml where it is present,
    # otherwise one that states the reference's values
    yaml_path = os.path.join(REFERENCE_ROOT, "configs", name + ".yaml") if reference_available() else _write_yaml_pair(str(tmp_path), name, ref)
    from_yaml = type(mine).from_yaml(yaml_path, ["MODEL.ROI_HEADS.SCORE_THRESH_TEST", 0.3])
    assert from_yaml == mine


@pytest.mark.parametrize("name", CONFIGS)
def test_every_hard_wired_semantic_holds_in_the_reference(name):
    """_FIXED_KEYS = what the kernels implement (aligned=False ROIAlign, 1 class, k4 s2 deconv, x2 bilinear ...): the
    reference's effective value of each such key must be one of the implemented ones for every BASELINE config."""
    from densepose_torchscript_amd.config import _FIXED_KEYS
    ref = _reference_values(name)
    for key, allowed in _FIXED_KEYS.items():
        assert key in ref, "reference has no key %s" % key
        v = ref[key]
        v = list(v) if isinstance(v, (list, tuple)) else v
        assert any(v == (list(a) if isinstance(a, (list, tuple)) else a) for a in allowed), (name, key, v, allowed)
