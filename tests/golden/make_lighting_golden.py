"""Golden vectors for the lighting module (pano_nerf_amd.lighting) by IMPORTING the reference's own functions:
sample_dir_by_pano (utils/sampling.py:5-20), solid_angle_refinement (utils/surface_rendering.py:294-316) and the shading
output of surface_rendering (utils/surface_rendering.py:129-165) with a probe's pixels as the light directions.

Build container only (needs a checkout of the reference at REF); stores seeded inputs and the reference's outputs, no
reference code.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_lighting_golden.py
"""
import os
import sys
import types

sys.dont_write_bytecode = True
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
for name in ("cv2", "Imath"):
    sys.modules[name] = types.ModuleType(name)
_exr = types.ModuleType("OpenEXR")
_exr.InputFile = _exr.OutputFile = _exr.Header = object
sys.modules["OpenEXR"] = _exr

import numpy as np  # noqa: E402
import torch  # noqa: E402

from utils.sampling import sample_dir_by_pano  # noqa: E402
from utils.surface_rendering import solid_angle_refinement, surface_rendering  # noqa: E402

SIZES = ((8, 16), (16, 32))
B = 6  # probes per size, one normal each (surface_rendering takes one env per batch row)
rng = np.random.Generator(np.random.PCG64(31))
out = {}
for h, w in SIZES:
    k = f"{h}x{w}/"
    dirs, _, _ = sample_dir_by_pano((h, w))
    dirs = dirs.reshape(-1, 3).astype(np.float32)
    omega = solid_angle_refinement(h, w)  # [1, h w, 1] fp32
    # HDR probe radiance: mostly in [0, 2), a few bright pixels (a sun)
    env = rng.random((B, h * w, 3)) * 2.0
    env[rng.random(env.shape[:2]) < 0.02] *= 25.0
    env = torch.tensor(env.astype(np.float32))
    n = rng.standard_normal((B, 3))
    n = torch.tensor((n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32))
    albedo = torch.tensor(rng.random((B, 3)).astype(np.float32))
    l = torch.tensor(dirs)[None].expand(B, -1, -1).contiguous()
    v = torch.zeros(B, 3)
    _, _, _, shading = surface_rendering(env, albedo, n, None, l, v, omega, output_sd=True)
    out[k + "dirs"] = dirs
    out[k + "omega"] = omega.numpy().reshape(-1)
    out[k + "env"] = env.numpy()
    out[k + "normal"] = n.numpy()
    out[k + "shading"] = shading.numpy()
np.savez_compressed(os.path.join(HERE, "lighting_ref.npz"), **out)
print("wrote", os.path.join(HERE, "lighting_ref.npz"), sorted(out))
