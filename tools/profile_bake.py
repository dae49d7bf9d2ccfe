"""GPU cost of baking a model onto its own mesh (geometry.bake_textures / write_obj), stage by stage: for a 64^3 and a 128^3
extract_mesh of a seeded PanoMipNeRF at atlas sizes 1024 and 2048 (a seeded model's sigma is noise around one value and
its median level set crosses nearly every cube - 784 k faces at 64^3 - so the level is the lowest of the sigma quantiles
0.9, 0.99, 0.999, 0.9999 whose mesh fits the smallest atlas: what a user does, who bakes a coarse mesh) - the atlas kernels
(pn_atlas_uv + pn_atlas_texels), the field query at the owned texels (query_field: albedo + normal), the encoding of the
normals (pn_atlas_encode_normals), the quantiser (pn_atlas_quantize, albedo against the sRGB table + normal map linear) and
the file writing (write_obj: host zlib and text) - each as the median of --iters synchronised calls (host clock around a
device synchronise) and, for the device stages, the mean of a window of --window back-to-back calls between two device
events.  The comparison that matters: the four new kernels together against query_field on the same rows, same run.
method="ray" (one renderer ray per owned texel) is timed once per mesh at size 1024.  One JSON line per configuration.

    python tools/profile_bake.py
    python tools/profile_bake.py --resolutions 64 --sizes 1024 --no-files
"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pano_nerf_amd import _lib, geometry  # noqa: E402
from tools.profile_objects import setup, timed  # noqa: E402
from tools.profile_textures import windowed  # noqa: E402

BOUNDS = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--no-files", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    model = setup()
    st = lambda: _lib.stream(dev)
    for res in a.resolutions:
        sigma = geometry.density_grid(model, BOUNDS, res)
        flat = sigma.view(-1).float().sort().values
        room = 2 * (min(a.sizes) // geometry.ATLAS_MIN_CELL) ** 2
        for quantile in (0.9, 0.99, 0.999, 0.9999):
            level = float(flat[int(quantile * (flat.numel() - 1))])
            F = int(geometry.marching_tetrahedra(sigma, level, BOUNDS)[1].shape[0])
            if 0 < F <= room:
                break
        del sigma, flat
        ms_mesh, mesh = timed(lambda: geometry.extract_mesh(model, BOUNDS, res, level, colors=None), max(1, a.iters // 2))
        V, F = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
        for size in a.sizes:
            out = dict(resolution=res, level=level, level_quantile=quantile, vertices=V, faces=F, extract_mesh_ms=ms_mesh,
                       size=size, iters=a.iters, window=a.window)
            try:
                cell = geometry.atlas_cell(F, size)
            except ValueError as e:
                out["error"] = str(e)
                print(json.dumps(out), flush=True)
                continue
            out["cell"] = cell

            def atlas():
                at = geometry.triangle_atlas(mesh.faces, size)
                return at, geometry.atlas_texels(mesh.vertices, mesh.faces, at, mesh.normals)

            out["atlas_ms"], (at, tex) = timed(atlas, a.iters)
            out["atlas_window_ms"] = windowed(atlas, a.window)
            own = tex["face"].reshape(-1) >= 0
            idx = torch.nonzero(own).reshape(-1)
            M = int(idx.numel())
            out["owned_texels"], out["owned_share"] = M, M / float(size * size)
            pts = tex["points"].reshape(-1, 3)[idx]
            var3 = tex["var"].reshape(-1)[idx][:, None].expand(-1, 3).contiguous()
            query = lambda: geometry.query_field(model, pts, var3, outputs=("albedo", "normal"))
            out["query_field_ms"], q = timed(query, a.iters)
            out["query_field_window_ms"] = windowed(query, max(2, a.window // 5))
            world = torch.zeros(size * size, 3, device=dev)
            world[idx] = q["normal"]
            albedo = torch.zeros(size * size, 3, device=dev)
            albedo[idx] = q["albedo"]
            enc = torch.empty(size, size, 3, device=dev)
            encode = lambda: _lib.call("pn_atlas_encode_normals", size, cell, F, V, mesh.vertices.data_ptr(),
                                       mesh.faces.data_ptr(), at.uv.data_ptr(), tex["face"].data_ptr(),
                                       tex["normals_s"].data_ptr(), world.data_ptr(), enc.data_ptr(), st())
            out["encode_ms"], _ = timed(encode, a.iters)
            out["encode_window_ms"] = windowed(encode, a.window)
            quant = lambda: (geometry.quantize_image(albedo.view(size, size, 3), srgb=True), geometry.quantize_image(enc))
            out["quantize_ms"], _ = timed(quant, a.iters)
            out["quantize_window_ms"] = windowed(quant, a.window)

            def kernels():
                atlas()
                encode()
                quant()

            # back to back in one run: the four new kernels against the field query on the same rows
            out["atlas_kernels_window_ms"] = windowed(kernels, a.window)
            out["query_field_window2_ms"] = windowed(query, max(2, a.window // 5))
            out["kernels_share_of_query"] = out["atlas_kernels_window_ms"] / out["query_field_window2_ms"]
            bake = lambda: geometry.bake_textures(model, mesh, size=size, maps=("albedo", "normal"))
            out["bake_textures_ms"], baked = timed(bake, a.iters)
            out["texels_per_s"] = M / (1e-3 * out["bake_textures_ms"])
            if size == a.sizes[0]:
                t0 = time.perf_counter()
                geometry.bake_textures(model, mesh, size=size, maps=("radiance", "normal"), method="ray")
                torch.cuda.synchronize()
                out["bake_ray_method_ms"] = 1e3 * (time.perf_counter() - t0)
            if not a.no_files:
                with tempfile.TemporaryDirectory() as tmp:
                    for fmt in ("png", "exr"):
                        t0 = time.perf_counter()
                        files = geometry.write_obj(os.path.join(tmp, "scene.obj"), baked, image_format=fmt)
                        out[f"write_obj_{fmt}_ms"] = 1e3 * (time.perf_counter() - t0)
                        out[f"write_obj_{fmt}_bytes"] = sum(os.path.getsize(p) for p in files.values()) + \
                            os.path.getsize(os.path.join(tmp, "scene.obj"))
            del baked, tex, at, q, world, albedo, enc, pts, var3
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
