"""Fit loop: the reference's ``train.py`` + ``systems/*`` without Lightning.

    python -m pano_nerf_amd.train --data_path D --config C --out_dir O [--range 0 10] [KEY VAL ...]

``Trainer`` lifts the step ``bench.py`` times into the package: sample a batch from the scene's device pool, model
forward, tone-mapped loss, backward, one all-reduce of the flat gradient (``world > 1``), one Adam kernel with the
learning rate in a device scalar.  Nothing is read back per step; the loss comes to the host every
``log_every_n_step`` steps only (never when that is 0).

Up to 2048 rays per GPU (the crossover bench.py records) the whole step is captured into a HIP graph and replayed; the
capture is checked first - one replay against one eager step on the same generator state, loss and flat gradient to
1e-6 relative - and EVERY rank runs eagerly when any rank cannot replay.  The surface term changes the launch sequence,
so a run whose ``train.surface_start_step`` lies inside it keeps two graphs.  Capturing and checking leave parameters,
Adam state and generator states exactly as they found them.

Validation is ``PanoNeRFSystem.validation_step`` (systems/panonerf_system.py:77-131): ``render_image`` of every
held-out view, the reference's dump tree written from ``views.to_frame`` and the ``io_exr`` writers, plus a
``metrics.json`` (``evaluate_panorama`` per view and its mean) that the reference does not have.

Checkpoints carry the layout of a Lightning checkpoint of the reference - ``state_dict`` under ``mip_nerf.mlp.*``,
``optimizer_states[0]`` as ``torch.optim.Adam.state_dict()``, ``global_step`` - plus the generator states, so a resumed
eager run continues bit for bit; a checkpoint written by the reference loads the same way.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

from . import io_exr
from .config import finalize, load_config
from .dist import allreduce_flat_grad
from .loss import mip_loss, pano_loss
from .metrics import evaluate_panorama
from .optim import FlatAdam, mip_lr
from .rays import rearrange_render_image
from .renderer import render_image
from .views import to_frame

PREFIX = "mip_nerf.mlp."
GRAPH_MAX_RAYS = 2048  # bench.py: replay pays at 512 rays per GPU, is even at 1024 / 2048, and buys nothing above
RENDER_CHUNK = 32768   # renderer.py: val.chunk_size 512 was sized for a 2020 GPU's memory; same bits at any chunk size


def build_model(hparams):
    """The model of BaseSystem.__init__ (systems/base_system.py:19-55); keys the HIP path does not build are refused by
    the constructor's own NotImplementedError."""
    from .render import MipNeRF, PanoMipNeRF
    name = hparams["nerf.mlp_name"]
    if name not in ("panonerf", "mipnerf"):
        raise ValueError(f"nerf.mlp_name must be 'panonerf' or 'mipnerf', got {name!r}")
    cls, nc = (MipNeRF, 1) if name == "mipnerf" else (PanoMipNeRF, 5)
    h = hparams
    return cls(num_samples=h["nerf.num_samples"], num_levels=h["nerf.num_levels"],
               resample_padding=h["nerf.resample_padding"], stop_resample_grad=h["nerf.stop_resample_grad"],
               use_viewdirs=h["nerf.use_viewdirs"], disparity=h["nerf.disparity"], ray_shape=h["nerf.ray_shape"],
               min_deg_point=h["nerf.min_deg_point"], max_deg_point=h["nerf.max_deg_point"], deg_view=h["nerf.deg_view"],
               density_activation=h["nerf.density_activation"], density_noise=h["nerf.density_noise"],
               density_bias=h["nerf.density_bias"], rgb_activation=h["nerf.rgb_activation"],
               alb_activation=h["nerf.alb_activation"], rgb_padding=h["nerf.rgb_padding"],
               disable_integration=h["nerf.disable_integration"], append_identity=h["nerf.append_identity"],
               mlp_net_depth=h["nerf.mlp.net_depth"], mlp_net_width=h["nerf.mlp.net_width"],
               mlp_net_depth_condition=h["nerf.mlp.net_depth_condition"],
               mlp_net_width_condition=h["nerf.mlp.net_width_condition"], mlp_skip_index=h["nerf.mlp.skip_index"],
               mlp_num_rgb_channels=h["nerf.mlp.num_rgb_channels"], mlp_num_density_channels=nc,
               mlp_net_activation=h["nerf.mlp.net_activation"], mlp_name=name, num_env_samples=h["nerf.num_env_samples"])


# ------------------------------------------------------------------------------------------------------ checkpoints
def checkpoint_dict(mlp, exp_avg, exp_avg_sq, step, global_step, hparams=None, lr=None, rng=None):
    """Parameters and flat Adam moments -> a dict in the layout of the reference's Lightning checkpoints (tensors and
    plain containers only)."""
    offs = mlp._offsets
    flat = mlp.flat_params().detach().cpu()
    m, v = exp_avg.detach().cpu(), exp_avg_sq.detach().cpu()
    named = list(mlp.named_parameters())  # = the order of mlp.parameters(), Adam's parameter indices
    cut = lambda t, k, p: t[offs[k]:offs[k] + p.numel()].view(p.shape).clone()
    state = {i: {"step": torch.tensor(float(step)), "exp_avg": cut(m, k, p), "exp_avg_sq": cut(v, k, p)}
             for i, (k, p) in enumerate(named)} if step > 0 else {}
    group = {"lr": lr, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0, "amsgrad": False,
             "params": list(range(len(named)))}
    return {"state_dict": {PREFIX + k: cut(flat, k, p) for k, p in named},
            "optimizer_states": [{"state": state, "param_groups": [group]}],
            "global_step": int(global_step), "hyper_parameters": dict(hparams or {}), "rng_states": rng}


def flat_state_from_checkpoint(ckpt, mlp):
    """Checkpoint dict (this package's or a Lightning checkpoint of the reference) ->
    (flat_params, exp_avg, exp_avg_sq, step, global_step): flat fp32 CPU vectors in `mlp`'s block layout; Adam's
    per-parameter state is mapped through the parameter order of mlp.parameters().  A pure function of its inputs."""
    offs, total = mlp._offsets, mlp._total
    named = list(mlp.named_parameters())
    sd = ckpt["state_dict"]
    flat, m, v = (torch.zeros(total, dtype=torch.float32) for _ in range(3))
    for k, p in named:
        if PREFIX + k not in sd:
            raise KeyError(f"checkpoint has no {PREFIX + k}")
        t = sd[PREFIX + k]
        if tuple(t.shape) != tuple(p.shape):
            raise ValueError(f"{PREFIX + k} is {tuple(t.shape)}, the model's is {tuple(p.shape)}")
        flat[offs[k]:offs[k] + p.numel()] = t.detach().float().cpu().reshape(-1)
    step = 0
    opts = ckpt.get("optimizer_states") or []
    if opts and opts[0].get("state"):
        st, order = opts[0]["state"], opts[0]["param_groups"][0]["params"]
        if len(order) != len(named):
            raise ValueError(f"the optimizer holds {len(order)} parameters, the model {len(named)}")
        steps = set()
        for idx, (k, p) in zip(order, named):
            s = st[idx]
            m[offs[k]:offs[k] + p.numel()] = s["exp_avg"].detach().float().cpu().reshape(-1)
            v[offs[k]:offs[k] + p.numel()] = s["exp_avg_sq"].detach().float().cpu().reshape(-1)
            steps.add(int(s["step"]))
        if len(steps) != 1:
            raise ValueError(f"Adam's parameters disagree on the step: {sorted(steps)}")
        step = steps.pop()
    return flat, m, v, step, int(ckpt.get("global_step", 0))


# ----------------------------------------------------------------------------------------------------------- trainer
class Trainer:
    """hparams: the flat dict of `config.load_config` (put through `config.finalize` here if it was not yet); scene: a
    `data.PanoScene`.  `graph=None` decides replay from the rays per GPU; True / False force it.  A Trainer seeds and
    draws from the process-wide torch generators (host and device), like the reference's setup_seed: two Trainers
    stepped in turns in one process share their draws."""

    def __init__(self, hparams, scene, model=None, rank=0, world=1, graph=None):
        h = self.hparams = dict(hparams) if "save_dir" in hparams else finalize(hparams)
        if h["val.randomized"]:
            raise NotImplementedError("val.randomized: True - render_image renders with randomized=False, as both shipped yamls ask")
        if h["train.white_bkgd"] or h["val.white_bkgd"]:
            raise NotImplementedError("white_bkgd needs 4-channel files; no panorama scene has them")
        self.scene, self.rank, self.world = scene, int(rank), int(world)
        self.dev = scene.device
        self.is_mip = h["nerf.mlp_name"] == "mipnerf"
        torch.manual_seed(h["seed"])  # host and device generators: the initial weights
        self.model = (build_model(h) if model is None else model).to(self.dev)
        if self.world > 1:  # identical replicas
            import torch.distributed as dist
            dist.broadcast(self.model.mlp.flat_params(), 0)
        self.opt = FlatAdam(self.model.mlp, lr=h["optimizer.lr_init"])
        self.opt.step_dev_t = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.env = None if self.is_mip else scene.env_rays(h["nerf.num_ray_samples"])
        self.batch = int(h["train.batch_size"])  # per process, as under the reference's DDP
        self.lr_dev = torch.zeros(1, device=self.dev)
        self.global_step = 0
        self.use_ort = h["loss.ort_loss"] > 0
        self.want_graph = (self.batch <= GRAPH_MAX_RAYS) if graph is None else bool(graph)
        self._graphs = {}  # enable_surf -> (CUDAGraph, (loss, flat gradient)) or None (eager)
        self.replay_checks = {}
        self.log_every = int(h.get("log_every_n_step") or 0)
        self.losses = []  # (step, loss) at the logged steps
        self.verbose = False
        self._last_val = None
        every = h["val.check_every_n_epoch"]
        self.val_interval = max(1, int(every * 1000 / self.world)) if every else 0
        torch.manual_seed(h["seed"] + self.rank)  # every rank draws its own batch and jitter
        if h.get("checkpoint.resume_path"):
            self.load(h["checkpoint.resume_path"])

    # -------------------------------------------------------------------------------------------------------- step
    def lr(self, step):
        h = self.hparams
        return mip_lr(step, h["optimizer.lr_init"], h["optimizer.lr_final"], h["optimizer.max_steps"],
                      h["optimizer.lr_delay_steps"], h["optimizer.lr_delay_mult"])

    def _surf(self, step):
        h = self.hparams
        return bool(h["train.surface"]) and step >= h["train.surface_start_step"] and not self.is_mip

    def _fwd_bwd(self, surf):
        """Sample this rank's batch, render, loss, backward -> (loss, flat gradient)."""
        h = self.hparams
        rays, gt = self.scene.train.sample(self.batch)
        self.opt.zero_grad()
        if self.is_mip:
            outs = self.model(rays=rays, randomized=h["train.randomized"], white_bkgd=False, use_ort_loss=self.use_ort)
            loss, _ = mip_loss(outs, rays.lossmult, gt, h, use_ort=self.use_ort)
        else:
            outs = self.model(rays=rays, env_rays=self.env, randomized=h["train.randomized"], white_bkgd=False,
                              enable_surf=surf, use_ort_loss=self.use_ort)
            loss, _ = pano_loss(outs, rays.lossmult, gt, h, surface=surf)
        loss.backward()
        self.last_outputs = outs
        return loss.detach(), self.model.mlp.last_flat_grad

    def _snapshot(self):
        o = self.opt
        return (self.model.mlp.flat_params().clone(), o.exp_avg.clone(), o.exp_avg_sq.clone(), o.step_dev_t.clone(),
                o.step_count, torch.cuda.get_rng_state(self.dev), torch.get_rng_state())

    def _restore(self, snap):
        o = self.opt
        self.model.mlp.flat_params().copy_(snap[0])
        o.exp_avg.copy_(snap[1]); o.exp_avg_sq.copy_(snap[2]); o.step_dev_t.copy_(snap[3])
        o.step_count = snap[4]
        torch.cuda.set_rng_state(snap[5], self.dev)
        torch.set_rng_state(snap[6])
        self.model.mlp.note_raw_write()

    def _capture(self, surf):
        """Whole-step capture (Adam included when world == 1), as bench.py's try_capture: the verdict is collective - every
        rank reaches the same all-reduce whatever happened locally - and training state is restored afterwards."""
        dev, world = self.dev, self.world
        snap = self._snapshot()
        ok, why, check, g_, out = True, None, None, None, None
        self.lr_dev.fill_(self.lr(self.global_step))
        try:
            if os.environ.get("PN_TRAIN_FAIL_CAPTURE_RANK") == str(self.rank):  # test hook: raised before capture begins
                raise RuntimeError("forced capture failure on this rank (PN_TRAIN_FAIL_CAPTURE_RANK)")
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(2):
                    o = self._fwd_bwd(surf)
                    if world == 1:
                        self.opt.step_dev(o[1], self.lr_dev, grad_scale=1.0)
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            g_ = torch.cuda.CUDAGraph()
            # thread_local: a collective library's helper threads may touch HIP while we capture
            with torch.cuda.graph(g_, capture_error_mode="thread_local" if world > 1 else "global"):
                out = self._fwd_bwd(surf)
                if world == 1:
                    self.opt.step_dev(out[1], self.lr_dev, grad_scale=1.0)
            # one replay must reproduce one eager step on the same parameters and generator state
            self._restore(snap)
            l_e, g_e = self._fwd_bwd(surf)
            l_e, g_e = l_e.clone(), g_e.clone()
            self._restore(snap)
            g_.replay()
            torch.cuda.synchronize(dev)
            l_g, g_g = out
            scale = float(g_e.abs().max())
            diff = float((g_g - g_e).abs().max())
            ok = (bool(torch.isfinite(l_g)) and abs(float(l_g) - float(l_e)) <= 1e-6 * abs(float(l_e))
                  and diff <= 1e-6 * scale and scale > 0)
            check = {"loss_eager": float(l_e), "loss_replay": float(l_g), "max_grad_diff_over_max_grad": diff / max(scale, 1e-30)}
            if not ok:
                why = f"a replayed step does not reproduce the eager step ({check})"
        except Exception as e:  # this rank cannot replay: the others learn it through the verdict below
            ok, why, g_ = False, f"graph capture unavailable ({type(e).__name__}: {e})", None
            torch.cuda.synchronize(dev)
        self._restore(snap)
        flag = torch.tensor([1.0 if ok else 0.0], device=dev)
        if world > 1:
            import torch.distributed as dist
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)  # reached by every rank on every path
        ok_all = bool(flag.item() > 0.5)
        self.replay_checks[bool(surf)] = dict(check or {}, ok=ok_all, ok_this_rank=ok, reason=why)
        if not ok_all:
            print(f"[train] rank {self.rank}: {why or 'another rank cannot replay the step'}; every rank runs eagerly",
                  file=sys.stderr)
        self._graphs[bool(surf)] = (g_, out) if ok_all else None

    def training_step(self):
        """One step at self.global_step -> the loss (a device scalar; not read back here)."""
        step, surf = self.global_step, self._surf(self.global_step)
        ent = None
        if self.want_graph:
            if surf not in self._graphs:
                self._capture(surf)
            ent = self._graphs[surf]
        self.lr_dev.fill_(self.lr(step))
        if ent is not None:
            ent[0].replay()
            loss, g = ent[1]
            if self.world == 1:  # Adam is part of the graph
                self.opt.step_count += 1
                self.model.mlp.note_raw_write()
        else:
            loss, g = self._fwd_bwd(surf)
        if ent is None or self.world > 1:
            allreduce_flat_grad(g, self.world)
            self.opt.step_dev(g, self.lr_dev, grad_scale=1.0 / self.world)
        self.global_step = step + 1
        if self.log_every and step % self.log_every == 0:
            self.losses.append((step, float(loss)))
            if self.verbose and self.rank == 0:
                print(f"[train] step {step} loss {self.losses[-1][1]:.6f} lr {self.lr(step):.3e}", flush=True)
        return loss

    def fit(self, max_steps=None):
        """Train to `max_steps` (default optimizer.max_steps) from self.global_step: one validation of the first held-out
        view before the first step, one of every view each val.check_every_n_epoch x 1000 / world steps and at the end."""
        n = int(self.hparams["optimizer.max_steps"] if max_steps is None else max_steps)
        if self.scene.held_out:
            self.validate(self.global_step, views=[0], save=False)
        while self.global_step < n:
            self.training_step()
            if self.val_interval and self.global_step % self.val_interval == 0:
                self.validate(self.global_step)
        if self._last_val != self.global_step:
            self.validate(self.global_step)
        return self

    # -------------------------------------------------------------------------------------------------- validation
    def _render_mip(self, rays, h, w):
        """The chunk loop of MipNeRFSystem.render_image (systems/mipnerf_system.py:95-130) -> render_image's 9-tuple with
        the entries MipNeRF has."""
        chunks, _ = rearrange_render_image(rays, RENDER_CHUNK)
        rgb, dep = [], []
        with torch.no_grad():
            for c in chunks:
                _, (f_rgb, f_dep, *_) = self.model(rays=c, randomized=False, white_bkgd=False, use_ort_loss=False)
                rgb.append(f_rgb)
                dep.append(f_dep.reshape(-1, 1))
        img = lambda x: torch.cat(x, 0).reshape(1, h, w, -1).permute(0, 3, 1, 2)
        return (None, img(rgb), None, img(dep), None, None, None, None, None)

    def render_view(self, i):
        """render_image's 9-tuple of held-out view i (every rank takes part when world > 1)."""
        rays = self.scene.held_out[i][0]
        h, w = self.scene.h, self.scene.w
        if self.is_mip:
            return self._render_mip(rays, h, w)
        return render_image(self.model, rays, self.env, h, w, chunk_size=RENDER_CHUNK, rank=self.rank, world=self.world)

    def validate(self, step, views=None, save=True):
        """Render, dump and score the held-out views -> {"step", "views": [metrics per view], "mean"}; rank 0 writes
        <save_dir>/val_{step:06d}/ and (save=True) checkpoints/last.ckpt."""
        h = self.hparams
        near, far = self.scene.near, self.scene.far
        out = os.path.join(h["save_dir"], f"val_{step:06d}")
        chw = lambda x: None if x is None else x.permute(0, 3, 1, 2).contiguous()
        per_view = []
        for i in (range(len(self.scene.held_out)) if views is None else views):
            _, hdr, depth, normal, albedo = self.scene.held_out[i]
            hdr, depth, normal, albedo = chw(hdr), chw(depth), chw(normal), chw(albedo)
            render = self.render_view(i)
            per_view.append(evaluate_panorama(render, hdr, None if self.is_mip else depth, None if self.is_mip else normal,
                                              None if self.is_mip else albedo))
            if self.rank != 0:
                continue
            _, p_hdr, _, p_dep, p_nor, p_alb, _, p_surf, _ = render
            exrs = {"gt_hdr": hdr, "pred_hdr": p_hdr, "pred_hdr_surf": p_surf}
            pngs = {"gt_ldr": (hdr, "ldr_gt"), "pred_ldr": (p_hdr, "ldr"), "pred_ldr_surf": (p_surf, "ldr"),
                    "gt_normal": (normal, "normal"), "pred_normal": (p_nor, "normal"), "gt_depth": (depth, "depth"),
                    "pred_depth": (p_dep, "depth"), "pred_albedo": (p_alb, "albedo")}
            for name, x in exrs.items():
                if x is not None:
                    os.makedirs(os.path.join(out, name), exist_ok=True)
                    io_exr.write_exr(os.path.join(out, name, f"{i:03d}.exr"),
                                     np.ascontiguousarray(x[0].permute(1, 2, 0).float().cpu().numpy()))
            for name, (x, kind) in pngs.items():
                if x is not None:
                    os.makedirs(os.path.join(out, name), exist_ok=True)
                    io_exr.write_png(os.path.join(out, name, f"{i:03d}.png"), to_frame(x, kind, near, far).cpu().numpy())
        keys = per_view[0].keys() if per_view else ()
        res = {"step": int(step), "views": per_view,
               "mean": {k: float(np.mean([m[k] for m in per_view])) for k in keys}}
        if self.rank == 0:
            os.makedirs(out, exist_ok=True)
            with open(os.path.join(out, "metrics.json"), "w") as fp:
                json.dump(res, fp, indent=1)
            if save:
                self.save(os.path.join(h["save_dir"], "checkpoints", "last.ckpt"))
        self._last_val = step
        self.last_metrics = res
        return res

    # ------------------------------------------------------------------------------------------------- checkpoints
    def state(self):
        o = self.opt
        rng = {"cuda": torch.cuda.get_rng_state(self.dev), "cpu": torch.get_rng_state()}
        return checkpoint_dict(self.model.mlp, o.exp_avg, o.exp_avg_sq, int(o.step_dev_t.item()), self.global_step,
                               self.hparams, self.lr(self.global_step), rng)

    def save(self, path):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        torch.save(self.state(), path)

    def load(self, path):
        ckpt = torch.load(path, map_location="cpu", weights_only=False) if isinstance(path, (str, os.PathLike)) else path
        flat, m, v, step, gstep = flat_state_from_checkpoint(ckpt, self.model.mlp)
        o = self.opt
        self.model.mlp.flat_params().copy_(flat.to(self.dev))
        self.model.mlp.note_raw_write()
        o.exp_avg.copy_(m.to(self.dev)); o.exp_avg_sq.copy_(v.to(self.dev))
        o.step_dev_t.fill_(step)
        o.step_count = step
        self.global_step = gstep
        rng = ckpt.get("rng_states")
        if rng:  # (a checkpoint of the reference has none: the run continues on fresh draws)
            torch.cuda.set_rng_state(rng["cuda"].cpu(), self.dev)
            torch.set_rng_state(rng["cpu"].cpu())
        return self


# ------------------------------------------------------------------------------------------------------ command line
def main(argv=None):
    ap = argparse.ArgumentParser(description="Train Pano-NeRF / mip-NeRF on a scene folder (the reference's train.py).")
    ap.add_argument("--data_path", required=True, help="scene folder with <meta_file>.json and the EXR materials")
    ap.add_argument("--out_dir", default="./exps/")
    ap.add_argument("--range", nargs=2, type=float, default=[0, 10], help="near far")
    ap.add_argument("--config", default=None, help="yaml file (default: the panonerf settings)")
    ap.add_argument("--meta_file", default="transforms_all")
    ap.add_argument("--normalize_depth", action="store_true")
    ap.add_argument("opts", nargs=argparse.REMAINDER, help="KEY VAL pairs overriding the config")
    args = ap.parse_args(argv)
    hp = finalize(load_config(args.config, args.opts), out_dir=args.out_dir, data_path=args.data_path,
                  range=list(args.range), meta_file=args.meta_file)
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    backend = os.environ.get("PN_TRAIN_BACKEND", "nccl")  # gloo: rehearsal on fewer GPUs than ranks
    if backend != "nccl":
        local %= max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    from .data import PanoScene
    scene = PanoScene(args.data_path, factor=hp["train.factor"], train_views=hp["train.sample_num"], near=args.range[0],
                      far=args.range[1], normalize_depth=args.normalize_depth, meta_file=args.meta_file, device=dev,
                      white_bkgd=hp["train.white_bkgd"])
    trainer = Trainer(hp, scene, rank=rank, world=world)
    trainer.verbose = True
    trainer.fit()
    if rank == 0:
        print(json.dumps({"save_dir": hp["save_dir"], "global_step": trainer.global_step,
                          "metrics": trainer.last_metrics["mean"] if scene.held_out else None}), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
