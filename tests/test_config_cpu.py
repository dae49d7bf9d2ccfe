"""pano_nerf_amd.config against the reference's own loader (tests/golden/make_config_golden.py -> config_ref.json) and
the train.py:51-57 fix-ups."""
import json
import os

import pytest

from pano_nerf_amd import config as cfgmod
from pano_nerf_amd import load_config

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF = json.load(open(os.path.join(GOLD, "config_ref.json")))


def _same(got, want):
    assert set(got) == set(want), set(got) ^ set(want)
    for k, (tname, val) in want.items():
        assert type(got[k]).__name__ == tname, (k, type(got[k]).__name__, tname)
        assert (list(got[k]) if isinstance(got[k], tuple) else got[k]) == val, (k, got[k], val)


@pytest.mark.parametrize("name", ["panonerf", "mipnerf"])
def test_yaml_matches_reference_loader(name):
    got = load_config(os.path.join(GOLD, name + ".yaml"))
    assert len(got) == 60
    _same(got, REF[name])
    assert got["optimizer.lr_init"] == 2e-4 and got["checkpoint.resume_path"] is None
    assert got["nerf.append_identity"] == "Ture"


def test_overrides_match_reference_merge():
    got = load_config(os.path.join(GOLD, "panonerf.yaml"), REF["overrides"])
    _same(got, REF["panonerf_overridden"])
    assert got["train.sample_num"] == (1, 2, 3) and got["train.randomized"] is False and got["brand.new_key"] == 7
    with pytest.raises(ValueError):
        load_config(None, ["lonely.key"])


def test_defaults_are_the_panonerf_yaml():
    _same(load_config(), REF["panonerf"])


def test_finalize():
    c = cfgmod.finalize(load_config(os.path.join(GOLD, "mipnerf.yaml")), out_dir="/x/out", data_path="/d", range=[0, 10])
    assert c["train.sample_num"] == [45, 46, 72]
    assert c["train.surface_start_step"] == 0.4 * 44000
    assert c["exp_name"] == "mipnerf_45_46_72" and c["save_dir"] == os.path.join("/x/out", "mipnerf_45_46_72")
    assert c["data_path"] == "/d" and c["range"] == [0, 10]
    c = cfgmod.finalize(load_config(None, ["train.surface_start_step", "3"]))
    assert c["train.surface_start_step"] == 3 and c["save_dir"] == os.path.join("./exps/", "panonerf_45_46_72")
