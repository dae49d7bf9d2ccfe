"""pano_nerf_amd — MI355X-native Pano-NeRF volumetric-rendering hot path.

Public surface (mirrors the reference's names):
    PanoMipNeRF, MipNeRF          models/pano_mip_nerf.py:117, models/mip_nerf.py:105
    Rays, rearrange_render_image  datasets/base_datasets.py:13-16, models/mip.py:530-547
    generate_pano_rays, generate_lit_rays   datasets/pano_datasets.py:152-263
    pano_loss, mip_loss           systems/panonerf_system.py:15-75, systems/mipnerf_system.py:22-53
    FlatAdam, mip_lr              systems/base_system.py:82-87, utils/lr_schedule.py:51-59
    render_image                  systems/panonerf_system.py:133-192
    metrics, io_exr               utils/metrics.py (calc_* / calc_ws_*, SSIM, depth, calc_simse), utils/io_exr.py:6-47
    evaluate_panorama             every metric of one render_image output against its ground truths (HIP kernels)
    geometry                      field queries (sigma, albedo, rgb, normal at 3-D points), sigma volumes, marching-tetrahedra
                                  meshes and PLY output of a trained model; bake_textures / write_obj / export_scene: the
                                  field baked onto a mesh as albedo and normal maps over a per-triangle atlas (HIP kernels)
    extract_mesh                  Mesh(vertices, faces, normals, colors) of {sigma > level} over a box
    lighting                      spatially-varying lighting: HDR light probes, SH projection, exact and SH irradiance,
                                  the model's own irradiance estimate at any point and SH irradiance volumes (HIP kernels)
    ibl                           light probes baked into engine-ready image-based lighting: GGX-prefiltered specular cube-map
                                  mips, irradiance cubes, the split-sum BRDF table, EXR export and ibl_shade (HIP kernels)
    views                         novel views: perspective cameras and ray pools, camera paths, render_view / render_path
                                  and the reference's viewable uint8 frames, reprojection between cameras and depth-aware
                                  warping of rendered frames to other poses: warp_view, render_path_warped (HIP kernels)
    objects                       virtual object insertion: ray / triangle tracing, the reference's Lambertian and microfacet
                                  shading under light probes, cast shadows, insert_object / insert_path (HIP kernels)
    relight                       virtual point and spot lights on rendered views: shadow maps rendered from the model's own
                                  depth, per-pixel visibility and Lambert shading, relight_view / relight_path (HIP kernel)
    emitters                      the captured scene's own light sources: connected bright regions of HDR probes (wrapped
                                  8-connectivity), their flux, direction and distance, as relight.PointLight objects and a
                                  KHR_lights_punctual-style JSON, and the residual environment without them (HIP kernels)
    fusion                        TSDF fusion: rendered (or captured) depth of posed panorama, pinhole, cube-map and fisheye
                                  views integrated into a signed distance volume, and the mesh of its zero crossing with
                                  the field's normals and colours: TSDFVolume, fuse_views, fused_mesh (HIP kernel)
    meshops                       cleaning exported meshes: connected components and debris removal, quadric vertex
                                  clustering with the face count as a target, and an honest edge census (HIP kernels)
    meshdist                      distances between surfaces: the closest point of a mesh to arbitrary points through the BVH,
                                  area-weighted surface samples, Chamfer / Hausdorff / F-score / normal consistency of two
                                  meshes and unsigned distance grids (HIP kernels)
    winding                       generalized winding numbers of open or closed meshes: a robust inside test, signed
                                  distance and its grids, and a watertight remesh of what a mesh encloses: winding_number,
                                  inside, signed_distance, remesh (HIP kernels)
    volume                        the field baked into a radiance volume (density, SH radiance, albedo / normal attributes) and
                                  marched with no network in the loop, with brick skipping: RadianceVolume, bake_volume,
                                  march_rays, render_volume, render_volume_path, volume_probes; and its sparse form, a brick
                                  table and a pool of the occupied bricks in fp32 or fp16, packed from a dense volume or
                                  baked directly and marched in place: SparseRadianceVolume, load_volume (HIP kernels)
    data, PanoScene               scene folders: transforms_all.json, train / held-out split, pose conversion and the EXR
                                  materials ingested on the device (datasets/pano_datasets.py:49-131; HIP kernel)
    load_config                   the flat dotted-key hyper-parameter dict of configs/config.py (yaml + KEY VAL overrides)
    Trainer                       the fit loop of train.py / systems/*: step, graph replay, validation dumps, metrics,
                                  checkpoints, resume, data-parallel ranks (python -m pano_nerf_amd.train)
    concurrent_step               one training step as concurrent sub-batches on separate HIP streams
    install                       register PanoMipNeRF / MipNeRF under the reference's import paths (zero-edit drop-in)
"""
__version__ = "0.1.0"

from .rays import (Rays, Rays_keys, namedtuple_map, rearrange_render_image, generate_pano_rays, generate_lit_rays,  # noqa
                   DeviceRayPool)
from .render import PanoMipNeRF, MipNeRF  # noqa
from .loss import pano_loss, mip_loss  # noqa
from .optim import FlatAdam, mip_lr  # noqa
from .renderer import render_image  # noqa
from . import metrics, io_exr  # noqa
from .metrics import evaluate_panorama  # noqa
from . import geometry  # noqa
from .geometry import extract_mesh  # noqa
from . import lighting  # noqa
from . import ibl  # noqa
from . import views  # noqa
from . import objects  # noqa
from . import relight  # noqa
from . import emitters  # noqa
from . import fusion  # noqa
from .fusion import TSDFVolume, fuse_views, fused_mesh  # noqa
from . import meshops  # noqa
from .meshops import mesh_components, filter_components, simplify_mesh  # noqa
from . import meshdist  # noqa
from .meshdist import closest_point, sample_surface, compare_meshes  # noqa
from . import winding  # noqa
from .winding import winding_number, signed_distance, remesh  # noqa
from . import volume  # noqa
from .volume import (RadianceVolume, SparseRadianceVolume, bake_volume, load_volume, march_rays, render_volume,  # noqa
                     volume_probes)
from . import data  # noqa
from .data import PanoScene  # noqa
from .config import load_config  # noqa
from .parallel import concurrent_step  # noqa
from .install import install, uninstall  # noqa


def __getattr__(name):
    # `train` is also a program (python -m pano_nerf_amd.train): it is imported on first use, not with the package
    if name in ("Trainer", "train"):
        import importlib
        mod = importlib.import_module(".train", __name__)
        return mod.Trainer if name == "Trainer" else mod
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
