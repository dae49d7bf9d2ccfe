"""Golden for pano_nerf_amd.config by RUNNING the reference's own loader (configs/config.py: load, merge_from_list) on
its two shipped yaml files and on an override list that exercises a float, a bool, a tuple, a string and a new key.

Stores the resulting flat dicts as {name: {key: [type name, value]}} (JSON cannot tell a tuple from a list or carry the
type of a number) and copies the two yaml files - settings only - beside it, so the test needs no reference checkout.

Build container only (needs a checkout of the reference at REF); no reference code is stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_config_golden.py
"""
import contextlib
import io
import json
import os
import shutil
import sys

sys.dont_write_bytecode = True
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)

from configs import config as rc  # noqa: E402

OVERRIDES = ["optimizer.lr_init", "5e-4", "train.randomized", "False", "train.sample_num", "[1, 2, 3]",
             "nerf.mlp_name", "mipnerf", "brand.new_key", "7", "train.surface_start_step", "0.25"]


def typed(d):
    return {k: [type(v).__name__, list(v) if isinstance(v, tuple) else v] for k, v in d.items()}


out = {"overrides": OVERRIDES}
for name in ("panonerf", "mipnerf"):
    src = os.path.join(REF, "configs", name + ".yaml")
    shutil.copyfile(src, os.path.join(HERE, name + ".yaml"))
    out[name] = typed(rc.load(src))
merged = rc.load(os.path.join(REF, "configs", "panonerf.yaml"))
with contextlib.redirect_stdout(io.StringIO()):  # ("[Error] New args ... is added")
    rc.merge_from_list(merged, OVERRIDES)
out["panonerf_overridden"] = typed(merged)
with open(os.path.join(HERE, "config_ref.json"), "w") as fp:
    json.dump(out, fp, indent=1, sort_keys=True)
print({k: len(v) for k, v in out.items()})
