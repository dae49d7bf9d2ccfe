"""The zero-edit integration route of INTEGRATION.md: with the upstream tree and this repository on sys.path and
`pano_nerf_amd.install()` called, every module that systems/base_system.py:1-6 and systems/panonerf_system.py:2-11 import
resolves — the two model modules to the MI355X classes, everything else to the upstream tree's own code.  The upstream tree is
a stand-in written from tests/golden/dropin_layout.json (its packages and modules, what the two systems import from them, the
keyword arguments base_system.py builds the model with; tests/golden/make_dropin_golden.py).  Runs in a subprocess (it
rearranges sys.path / sys.modules)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUT = os.path.join(ROOT, "tests", "golden", "dropin_layout.json")


def write_stand_in(root, layout):
    """The upstream tree's layout under `root`: a module per upstream module, defining the names the two systems import from
    it; systems/base_system.py builds the model with the upstream keyword arguments, systems/panonerf_system.py makes the
    upstream imports."""
    wanted = {}
    for imports in layout["system_imports"].values():
        for mod, names in imports:
            wanted.setdefault(mod, set()).update(n for n in names if n != "*")
    for pkg, info in layout["packages"].items():
        os.makedirs(os.path.join(root, pkg))
        if info["regular"]:
            open(os.path.join(root, pkg, "__init__.py"), "w").close()
        for m in info["modules"]:
            src = "".join(f"def {n}(*args, **kwargs):\n    raise NotImplementedError('stand-in')\n\n\n"
                          for n in sorted(wanted.get(f"{pkg}.{m}", ())))
            with open(os.path.join(root, pkg, m + ".py"), "w") as f:
                f.write(src)

    def import_lines(mod, skip_models=False):
        return "".join(f"from {m} import {', '.join(names)}\n" for m, names in layout["system_imports"][mod]
                       if not (skip_models and m.startswith("models.")))
    with open(os.path.join(root, "systems", "base_system.py"), "w") as f:
        f.write("from pytorch_lightning import LightningModule\n" + import_lines("systems.base_system", skip_models=True) + f"""
KWARGS = {layout["model_kwargs"]!r}
DENSITY_CHANNELS = {layout["num_density_channels"]!r}


class BaseSystem(LightningModule):
    def __init__(self, hparams):
        super().__init__()
        self.save_hyperparameters(hparams)
        if hparams["nerf.mlp_name"] == "mipnerf":
            from models.mip_nerf import MipNeRF as NeRFModel
        else:
            from models.pano_mip_nerf import PanoMipNeRF as NeRFModel
        local = {{"num_density_channels": DENSITY_CHANNELS[hparams["nerf.mlp_name"]]}}
        self.mip_nerf = NeRFModel(**{{k: hparams[v["hparam"]] if "hparam" in v else local[v["local"]]
                                      for k, v in KWARGS.items()}})
""")
    with open(os.path.join(root, "systems", "panonerf_system.py"), "w") as f:
        f.write(import_lines("systems.panonerf_system"))


SCRIPT = r'''
import sys, types
sys.dont_write_bytecode = True
REF, ROOT = sys.argv[1], sys.argv[2]
sys.path[:0] = [REF, ROOT]          # exactly what INTEGRATION.md says: the upstream tree first, then this repository
# libraries the reference imports that this image lacks (as tests/golden/make_golden.py does); none is on the hot path
for name in ("cv2", "Imath", "lpips", "torchvision", "torchvision.utils", "wandb", "matplotlib", "matplotlib.pyplot",
             "matplotlib.cm"):
    if name not in sys.modules:
        try:
            __import__(name)
        except Exception:
            sys.modules[name] = types.ModuleType(name)
exr = types.ModuleType("OpenEXR"); exr.InputFile = exr.OutputFile = exr.Header = object
sys.modules.setdefault("OpenEXR", exr)
pl = types.ModuleType("pytorch_lightning")
import torch
class LightningModule(torch.nn.Module):
    def save_hyperparameters(self, h): self.hparams = dict(h)
pl.LightningModule = LightningModule
sys.modules["pytorch_lightning"] = pl

import pano_nerf_amd
pano_nerf_amd.install()
pano_nerf_amd.install()              # idempotent

import models.pano_mip_nerf, models.mip_nerf
assert models.pano_mip_nerf.PanoMipNeRF is pano_nerf_amd.PanoMipNeRF
assert models.mip_nerf.MipNeRF is pano_nerf_amd.MipNeRF
from models.pano_mip_nerf import PanoMipNeRF as A
from models.mip_nerf import MipNeRF as B
assert A is pano_nerf_amd.PanoMipNeRF and B is pano_nerf_amd.MipNeRF

# everything else the two systems import must still be the reference's own code
import importlib
for name in ("models.loss", "models.mip", "utils.surface_rendering", "utils.lr_schedule", "utils.metrics", "utils.io_exr",
             "datasets.pano_datasets", "datasets.base_datasets"):
    m = importlib.import_module(name)
    assert m.__file__.startswith(REF), (name, m.__file__)
import utils.surface_rendering as sr
assert sr.hdr_to_ldr.__module__ == "utils.surface_rendering" and sr.__file__.startswith(REF)
from models.mip import rearrange_render_image
assert rearrange_render_image.__module__ == "models.mip"
try:
    importlib.import_module("utils.vis")       # needs torchvision / cv2 functions only at call time
except Exception as e:
    print("utils.vis:", type(e).__name__, e)

# systems/base_system.py:10-55 — construct the system's model exactly as the reference does
import systems.base_system as bs
assert bs.__file__.startswith(REF)
hp = {"train.randomized": True, "val.randomized": False, "train.white_bkgd": False, "val.chunk_size": 512,
      "train.batch_size": 512, "nerf.mlp_name": "panonerf", "nerf.num_samples": 8, "nerf.num_levels": 2,
      "nerf.resample_padding": 0.01, "nerf.stop_resample_grad": True, "nerf.use_viewdirs": True, "nerf.disparity": False,
      "nerf.ray_shape": "cone", "nerf.min_deg_point": 0, "nerf.max_deg_point": 16, "nerf.deg_view": 4,
      "nerf.density_activation": "softplus", "nerf.density_noise": 0.0, "nerf.density_bias": -1.0,
      "nerf.rgb_activation": "softplus", "nerf.alb_activation": "sigmoid", "nerf.rgb_padding": 0.0,
      "nerf.disable_integration": False, "nerf.append_identity": "Ture", "nerf.mlp.net_depth": 8, "nerf.mlp.net_width": 256,
      "nerf.mlp.net_depth_condition": 1, "nerf.mlp.net_width_condition": 128, "nerf.mlp.skip_index": 4,
      "nerf.mlp.num_rgb_channels": 3, "nerf.mlp.net_activation": "relu", "nerf.num_env_samples": 10,
      "nerf.solid_angle_height": 8, "nerf.solid_angle_width": 16}
class _H(dict):
    def __missing__(self, k):  # keys of configs/panonerf.yaml this test does not spell out
        raise KeyError(k)
try:
    system = bs.BaseSystem(_H(hp))
except KeyError as e:
    print("MISSING_HPARAM", e); raise
assert type(system.mip_nerf) is pano_nerf_amd.PanoMipNeRF
keys = list(system.mip_nerf.state_dict().keys())
assert "mlp.layers.0.0.weight" in keys and "mlp.color_layer.bias" in keys and len(keys) == 24
opt = torch.optim.Adam(system.mip_nerf.mlp.parameters(), lr=2e-4)   # base_system.py:82
assert len(opt.param_groups[0]["params"]) == 24
import systems.panonerf_system as ps  # systems/panonerf_system.py:2-11 resolve with the drop-in installed
assert ps.BaseSystem is bs.BaseSystem and ps.rearrange_render_image is rearrange_render_image and ps.__file__.startswith(REF)
print("DROPIN_OK")
'''


def test_install_resolves_reference_imports(tmp_path):
    with open(LAYOUT) as f:
        write_stand_in(str(tmp_path), json.load(f))
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    res = subprocess.run([sys.executable, "-c", SCRIPT, str(tmp_path), ROOT], capture_output=True, text=True, timeout=300,
                         env=env)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert "DROPIN_OK" in res.stdout


def test_package_alias_is_a_real_package():
    sys.path.insert(0, ROOT)
    import pano_nerf_amd as pn
    assert pn.__spec__.name == "pano_nerf_amd" and pn.__file__.endswith(os.path.join("pano-nerf_amd", "__init__.py"))
    assert pn.render.PanoMipNeRF.__module__ == "pano_nerf_amd.render"
    assert callable(pn.install)
