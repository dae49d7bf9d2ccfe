"""Configuration: the flat dotted-key dict of the reference's ``configs/config.py`` and the fix-ups of ``train.py:51-57``.

``load_config(path, overrides)`` reads a nested yaml file, flattens it with ``.``, passes every string through
``ast.literal_eval`` where that succeeds and turns lists into tuples - which explains what the shipped yamls give:
``lr_init: 2e-4`` (a string to ``yaml.safe_load``) becomes a float, ``resume_path: None`` becomes ``None`` and
``append_identity: Ture`` stays the truthy string ``'Ture'``.  Trailing ``KEY VAL`` pairs override the file, parsed
the same way.  With no file the defaults below are used: the values of the reference's ``panonerf.yaml``.
"""
import ast
import os

DEFAULTS = {
    "seed": 4, "log_every_n_step": 1,
    "train.batch_size": 512, "train.batch_type": "all_images", "train.num_work": 28, "train.factor": 4,
    "train.randomized": True, "train.white_bkgd": False, "train.surface": True, "train.surface_start_step": 0,
    "train.sample_num": "n45_46_72", "train.sample_start": 0,
    "val.batch_size": 1, "val.batch_type": "single_image", "val.num_work": 28, "val.factor": 4, "val.randomized": False,
    "val.white_bkgd": False, "val.check_every_n_epoch": 10, "val.chunk_size": 512,
    "nerf.mlp_name": "panonerf", "nerf.num_env_samples": 10, "nerf.num_ray_samples": 10, "nerf.num_samples": 64,
    "nerf.num_levels": 2, "nerf.resample_padding": 0.01, "nerf.stop_resample_grad": True, "nerf.use_viewdirs": True,
    "nerf.disparity": False, "nerf.ray_shape": "cone", "nerf.min_deg_point": 0, "nerf.max_deg_point": 16,
    "nerf.deg_view": 4, "nerf.density_activation": "softplus", "nerf.density_noise": 0.0, "nerf.density_bias": -1.0,
    "nerf.rgb_activation": "softplus", "nerf.alb_activation": "sigmoid", "nerf.rgb_padding": 0,
    "nerf.disable_integration": False, "nerf.append_identity": "Ture",
    "nerf.mlp.num_density_channels": 5, "nerf.mlp.net_depth": 8, "nerf.mlp.net_width": 256,
    "nerf.mlp.net_depth_condition": 1, "nerf.mlp.net_width_condition": 128, "nerf.mlp.net_activation": "relu",
    "nerf.mlp.skip_index": 4, "nerf.mlp.num_rgb_channels": 3,
    "optimizer.lr_init": 2e-4, "optimizer.lr_final": 2e-5, "optimizer.lr_delay_steps": 120,
    "optimizer.lr_delay_mult": 0.01, "optimizer.max_steps": 44000,
    "loss.disable_multiscale_loss": False, "loss.coarse_loss_mult": 0.1, "loss.surface_loss": 1, "loss.ort_loss": 0.1,
    "loss.chrom_loss": 0.1,
    "checkpoint.resume_path": None,
}


def _parse(value):
    if isinstance(value, str):
        try:
            value = ast.literal_eval(value)
        except (ValueError, SyntaxError):
            pass  # really a string
    if isinstance(value, list):
        value = tuple(value)
    return value


def flatten(tree, prefix=""):
    """Nested dict -> {'a.b.c': parsed value}."""
    out = {}
    for k, v in (tree or {}).items():
        if isinstance(v, dict):
            out.update(flatten(v, prefix + k + "."))
        else:
            out[prefix + k] = _parse(v)
    return out


def load_config(path=None, overrides=()):
    """-> flat dict of hyper-parameters: `path` (yaml) or the panonerf defaults, then the `KEY VAL` pairs of `overrides`."""
    if path is None:
        cfg = dict(DEFAULTS)
    else:
        import yaml
        with open(path) as fp:
            cfg = flatten(yaml.safe_load(fp))
    overrides = list(overrides)
    if len(overrides) % 2:
        raise ValueError("overrides must be KEY VAL pairs")
    for k, v in zip(overrides[0::2], overrides[1::2]):
        cfg[k] = _parse(v)
    return cfg


def finalize(cfg, out_dir="./exps/", **extra):
    """The fix-ups of train.py:51-57 on a copy of `cfg`: `train.sample_num` 'n45_46_72' -> [45, 46, 72]; a fractional
    `train.surface_start_step` times `optimizer.max_steps`; `exp_name` and `save_dir = out_dir / <mlp_name>_<ids>`.
    `extra` are the command line's own entries (data_path, range, ...): added where the config does not set them."""
    cfg = dict(cfg)
    for k, v in dict(extra, out_dir=out_dir).items():
        cfg.setdefault(k, v)
    if isinstance(cfg["train.sample_num"], str):
        cfg["train.sample_num"] = [int(x) for x in cfg["train.sample_num"][1:].split("_")]
    cfg["exp_name"] = f"{cfg['nerf.mlp_name']}_{'_'.join(str(x) for x in cfg['train.sample_num'])}"
    if 0 < cfg["train.surface_start_step"] < 1:
        cfg["train.surface_start_step"] = cfg["train.surface_start_step"] * cfg["optimizer.max_steps"]
    cfg["save_dir"] = os.path.join(cfg["out_dir"], cfg["exp_name"])
    return cfg
