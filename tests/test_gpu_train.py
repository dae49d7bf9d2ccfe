"""The fit loop (pano_nerf_amd.train) on a small synthetic scene folder written by the test: 3 training views and 1
held-out view at 32 x 64 of the oracle's analytic radiance (test data only: no product path imports the oracle), depth /
normal / albedo as seeded arrays, files a mix of ZIP / HALF and uncompressed / FLOAT; 32 samples, batches of 256 rays.

Held-out LDR PSNR and training loss after 300 steps are recorded in profiles/train_fit_synthetic.txt; this file checks a
direction only (tests/test_gpu_psnr.py pins the trajectory against the reference's ensemble)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pano_nerf_amd as pn
from pano_nerf_amd import config, io_exr, train
from oracle import pano_oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
H, W, B = 32, 64, 256
OVERRIDES = ["train.factor", "1", "train.sample_num", "[0, 1, 2]", "nerf.num_samples", "32", "train.batch_size", str(B)]
EXR_DIRS = {"gt_hdr", "pred_hdr", "pred_hdr_surf"}
PNG_DIRS = {"gt_ldr", "pred_ldr", "pred_ldr_surf", "gt_normal", "pred_normal", "gt_depth", "pred_depth", "pred_albedo"}


def write_scene(folder):
    os.makedirs(folder, exist_ok=True)
    _, rgbs, _, c2ws = orc.synthetic_scene(H, W, 4, seed=4)
    images = rgbs.numpy().reshape(4, H, W, 3)
    rng = np.random.default_rng(8)
    normal = rng.standard_normal((4, H, W, 3))
    normal /= np.linalg.norm(normal, axis=-1, keepdims=True)
    mats = {"image": images, "albedo": rng.uniform(0, 1, (4, H, W, 3)), "normal": (normal + 1) / 2,
            "depth": rng.uniform(1, 5, (4, H, W, 1))}
    formats = [dict(compression="zip", half=True), dict(), dict(compression="zips", half=True), dict(compression="zip")]
    b2w = np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])  # R_x(pi / 2): the loader multiplies positions by it
    meta = {}
    for mat, arr in mats.items():
        meta[mat] = []
        for i in range(4):
            m = np.eye(4)
            m[:3, 3] = c2ws[i][:3, 3].astype(np.float64) @ b2w.T
            name = f"{mat}/{i:03d}"
            os.makedirs(os.path.join(folder, mat), exist_ok=True)
            io_exr.write_exr(os.path.join(folder, name + ".exr"), arr[i].astype(np.float32), **formats[i])
            meta[mat].append({"file_path": name, "transform_matrix": m.tolist()})
    with open(os.path.join(folder, "transforms_all.json"), "w") as fp:
        json.dump(meta, fp)
    return folder


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return write_scene(str(tmp_path_factory.mktemp("data") / "scene"))


@pytest.fixture(scope="module")
def scene(scene_dir):
    s = pn.PanoScene(scene_dir, factor=1, train_views=[0, 1, 2], keep_rotation=False, pano_normals=False)
    assert (s.h, s.w) == (H, W) and len(s.held_out) == 1 and len(s.train) == 3 * H * W
    _, _, _, c2ws = orc.synthetic_scene(H, W, 4, seed=4)
    assert np.abs(s.train.c2ws_host - np.stack(c2ws[:3])).max() <= 1e-6
    return s


def hparams(tmp_path, *extra, cfg=None):
    return config.finalize(pn.load_config(cfg, OVERRIDES + [str(x) for x in extra]), out_dir=str(tmp_path))


def hand_loop(hp, scene, steps, surf_from=0):
    """The step written out with the public pieces, under the same seed: batch indices first, then the model's draws."""
    dev = scene.device
    torch.manual_seed(hp["seed"])
    model = train.build_model(hp).to(dev)
    opt = pn.FlatAdam(model.mlp, lr=hp["optimizer.lr_init"])
    env = scene.env_rays(hp["nerf.num_ray_samples"])
    lr_dev = torch.zeros(1, device=dev)
    torch.manual_seed(hp["seed"])
    losses = []
    for i in range(steps):
        rays, gt = scene.train.sample(B)
        opt.zero_grad()
        surf = i >= surf_from
        outs = model(rays=rays, env_rays=env, randomized=True, white_bkgd=False, enable_surf=surf, use_ort_loss=True)
        loss, _ = pn.pano_loss(outs, rays.lossmult, gt, hp, surface=surf)
        loss.backward()
        lr_dev.fill_(pn.mip_lr(i, hp["optimizer.lr_init"], hp["optimizer.lr_final"], hp["optimizer.max_steps"],
                               hp["optimizer.lr_delay_steps"], hp["optimizer.lr_delay_mult"]))
        opt.step_dev(model.mlp.last_flat_grad, lr_dev, grad_scale=1.0)
        losses.append(float(loss))
    return losses, model, opt


def close(a, b, what):
    worst = max(abs(x - y) / abs(y) for x, y in zip(a, b))
    print(f"{what}: worst relative loss difference {worst:.2e}")
    assert len(a) == len(b) and worst <= 1e-6, (what, worst, a, b)


def test_fit_matches_hand_loop(tmp_path, scene):
    hp = hparams(tmp_path, "log_every_n_step", 1)
    tr = pn.Trainer(hp, scene, graph=False).fit(20)
    assert [s for s, _ in tr.losses] == list(range(20)) and tr.global_step == 20
    want, model, opt = hand_loop(hp, scene, 20)
    close([l for _, l in tr.losses], want, "fit vs hand loop")
    assert torch.equal(tr.model.mlp.flat_params(), model.mlp.flat_params())
    assert os.path.isfile(os.path.join(hp["save_dir"], "checkpoints", "last.ckpt"))
    assert sorted(d for d in os.listdir(hp["save_dir"]) if d.startswith("val_")) == ["val_000000", "val_000020"]


def test_no_readback_when_logging_is_off(tmp_path, scene):
    tr = pn.Trainer(hparams(tmp_path, "log_every_n_step", 0), scene, graph=False)
    for _ in range(3):
        out = tr.training_step()
    assert tr.losses == [] and out.is_cuda and out.dim() == 0
    tr = pn.Trainer(hparams(tmp_path, "log_every_n_step", 2), scene, graph=False)
    for _ in range(5):
        tr.training_step()
    assert [s for s, _ in tr.losses] == [0, 2, 4]


def test_graph_replay_matches_eager(tmp_path, scene):
    hp = hparams(tmp_path, "log_every_n_step", 1)
    assert pn.Trainer(hp, scene).want_graph and not pn.Trainer(hparams(tmp_path, "train.batch_size", 4096), scene).want_graph
    # one after the other: a Trainer seeds and draws from the process-wide generators
    eager = pn.Trainer(hp, scene, graph=False)
    for _ in range(5):
        eager.training_step()
    graph = pn.Trainer(hp, scene, graph=True)
    for _ in range(5):
        graph.training_step()
    chk = graph.replay_checks[True]
    print("replay check:", chk)
    assert chk["ok"] and chk["ok_this_rank"] and chk["max_grad_diff_over_max_grad"] <= 1e-6
    assert graph._graphs[True] is not None and list(graph._graphs) == [True]
    close([l for _, l in graph.losses], [l for _, l in eager.losses], "graph vs eager")
    assert int(graph.opt.step_dev_t.item()) == 5 == graph.opt.step_count


def test_surface_switch(tmp_path, scene):
    hp = hparams(tmp_path, "log_every_n_step", 1, "train.surface_start_step", 3)
    tr = pn.Trainer(hp, scene, graph=False)
    for _ in range(7):
        tr.training_step()
    got = [l for _, l in tr.losses]
    want, _, _ = hand_loop(hp, scene, 7, surf_from=3)
    close(got, want, "surface from step 3")
    never, _, _ = hand_loop(hp, scene, 4, surf_from=99)
    close(got[:3], never[:3], "steps 0-2 carry no surface term")
    assert abs(got[3] - never[3]) > 1e-4 * abs(never[3])  # ... and step 3 does
    # graph replay keeps one graph per launch sequence
    g = pn.Trainer(hp, scene, graph=True)
    for _ in range(7):
        g.training_step()
    assert set(g._graphs) == {False, True} and all(v is not None for v in g._graphs.values())
    assert g.replay_checks[False]["ok"] and g.replay_checks[True]["ok"]
    close([l for _, l in g.losses], got, "two graphs vs eager")


def test_resume_is_bit_identical(tmp_path, scene):
    hp = hparams(tmp_path, "log_every_n_step", 0)
    whole = pn.Trainer(hp, scene, graph=False)
    for _ in range(12):
        whole.training_step()
    first = pn.Trainer(hp, scene, graph=False)
    for _ in range(6):
        first.training_step()
    path = str(tmp_path / "mid.ckpt")
    first.save(path)
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert ckpt["global_step"] == 6 and "mip_nerf.mlp.layers.0.0.weight" in ckpt["state_dict"]
    assert ckpt["hyper_parameters"]["train.batch_size"] == B and int(ckpt["optimizer_states"][0]["state"][0]["step"]) == 6
    second = pn.Trainer(hparams(tmp_path, "log_every_n_step", 0, "seed", 99), scene, graph=False).load(path)
    assert second.global_step == 6
    for _ in range(6):
        second.training_step()
    assert torch.equal(second.model.mlp.flat_params(), whole.model.mlp.flat_params())
    assert torch.equal(second.opt.exp_avg, whole.opt.exp_avg) and torch.equal(second.opt.exp_avg_sq, whole.opt.exp_avg_sq)
    assert int(second.opt.step_dev_t.item()) == 12
    # checkpoint.resume_path is honoured
    third = pn.Trainer(hparams(tmp_path, "checkpoint.resume_path", path), scene, graph=False)
    assert third.global_step == 6 and torch.equal(third.model.mlp.flat_params(), first.model.mlp.flat_params())


def test_learning_direction(tmp_path, scene):
    hp = hparams(tmp_path, "log_every_n_step", 10)
    tr = pn.Trainer(hp, scene).fit(300)
    before = json.load(open(os.path.join(hp["save_dir"], "val_000000", "metrics.json")))
    after = json.load(open(os.path.join(hp["save_dir"], "val_000300", "metrics.json")))
    l0, l1 = np.mean([l for _, l in tr.losses[:3]]), np.mean([l for _, l in tr.losses[-3:]])
    print(f"held-out LDR PSNR: step 0 {before['mean']['ldr_psnr']:.3f} dB, step 300 {after['mean']['ldr_psnr']:.3f} dB; "
          f"training loss {l0:.5f} -> {l1:.5f}; launch: {'graph replay' if tr._graphs.get(True) else 'eager'}")
    assert after["mean"]["ldr_psnr"] > before["mean"]["ldr_psnr"]
    assert l1 < l0


def test_validation_outputs(tmp_path, scene):
    hp = hparams(tmp_path, "log_every_n_step", 0)
    tr = pn.Trainer(hp, scene, graph=False).fit(3)
    out = os.path.join(hp["save_dir"], "val_000003")
    assert set(os.listdir(out)) == EXR_DIRS | PNG_DIRS | {"metrics.json"}
    for d in EXR_DIRS:
        assert os.listdir(os.path.join(out, d)) == ["000.exr"], d
    for d in PNG_DIRS:
        assert os.listdir(os.path.join(out, d)) == ["000.png"], d
        assert open(os.path.join(out, d, "000.png"), "rb").read(8) == b"\x89PNG\r\n\x1a\n"
    rays, hdr, depth, normal, albedo = scene.held_out[0]
    render = pn.render_image(tr.model, rays, tr.env, H, W)
    for name, img in (("pred_hdr", render[1]), ("pred_hdr_surf", render[7]), ("gt_hdr", hdr.permute(0, 3, 1, 2))):
        back = io_exr.read_exr(os.path.join(out, name, "000.exr"))
        assert np.array_equal(back, img[0].permute(1, 2, 0).cpu().numpy()), name
    chw = lambda x: x.permute(0, 3, 1, 2).contiguous()
    want = pn.evaluate_panorama(render, chw(hdr), chw(depth), chw(normal), chw(albedo))
    got = json.load(open(os.path.join(out, "metrics.json")))
    assert got["step"] == 3 and len(got["views"]) == 1
    for k, v in want.items():
        assert got["views"][0][k] == v or (math.isnan(v) and math.isnan(got["views"][0][k])), k
        assert got["mean"][k] == v or math.isnan(v), k
    for k in ("psnr", "ldr_psnr", "ssim", "normal_mae", "depth_abs_rel", "albedo_psnr"):
        assert k in got["mean"], k
    with pytest.raises(NotImplementedError):
        pn.Trainer(hparams(tmp_path, "val.randomized", True), scene)
    with pytest.raises(NotImplementedError):
        pn.Trainer(hparams(tmp_path, "nerf.num_levels", 3), scene)  # the constructor's own refusal


def test_mipnerf_route(tmp_path, scene):
    hp = hparams(tmp_path, "log_every_n_step", 1, cfg=os.path.join(GOLD, "mipnerf.yaml"))
    assert hp["nerf.mlp_name"] == "mipnerf" and hp["train.surface_start_step"] == 0.4 * 44000
    tr = pn.Trainer(hp, scene, graph=False)
    assert isinstance(tr.model, pn.MipNeRF)
    for _ in range(10):
        tr.training_step()
    losses = [l for _, l in tr.losses]
    print("mipnerf losses:", losses)
    assert all(math.isfinite(l) for l in losses) and np.mean(losses[5:]) < np.mean(losses[:5])
    assert len(tr.last_outputs) == 2 and all(len(lvl) == 4 for lvl in tr.last_outputs)
    res = tr.validate(10)
    out = os.path.join(hp["save_dir"], "val_000010")
    assert set(os.listdir(out)) == {"gt_hdr", "pred_hdr", "gt_ldr", "pred_ldr", "gt_normal", "gt_depth", "pred_depth",
                                    "metrics.json"}
    assert {"psnr", "ws_psnr", "ldr_psnr", "ldr_ws_psnr"} <= set(res["mean"]) and "normal_mae" not in res["mean"]
    assert os.path.basename(hp["save_dir"]) == "mipnerf_0_1_2"


@pytest.mark.parametrize("mode", ["graph", "capture-fails-on-rank-1"])
def test_two_rank_rehearsal(tmp_path, scene_dir, mode):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    if mode != "graph":  # a Python exception raised before capture begins on ONE rank sends BOTH ranks to eager launches
        env["PN_TRAIN_FAIL_CAPTURE_RANK"] = "1"
    out = str(tmp_path / "out")
    os.makedirs(out)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", "29523", os.path.join(ROOT, "tests", "_train_dist_worker.py"), scene_dir, out]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=420, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    assert "TRAIN_DIST_OK" in res.stdout
    recs = {r: json.load(open(os.path.join(out, f"rank{r}.json"))) for r in (0, 1)}
    for r, rec in recs.items():
        chk = rec["check"]["true"]
        if mode == "graph":
            assert rec["replaying"] and chk["ok"] and chk["ok_this_rank"]
        else:
            assert not rec["replaying"] and not chk["ok"] and chk["ok_this_rank"] == (r == 0)
    assert "capture unavailable" in recs[1]["check"]["true"]["reason"] if mode != "graph" else True
    assert os.path.exists(os.path.join(out, "saved_by_rank0")) and not os.path.exists(os.path.join(out, "saved_by_rank1"))
    assert os.path.isfile(os.path.join(out, "panonerf_0_1_2", "checkpoints", "last.ckpt"))
    assert os.path.isfile(os.path.join(out, "panonerf_0_1_2", "val_000005", "metrics.json"))


def test_command_line(tmp_path, scene_dir):
    out = str(tmp_path / "exps")
    cmd = [sys.executable, "-m", "pano_nerf_amd.train", "--data_path", scene_dir, "--out_dir", out, "--range", "0", "10",
           *OVERRIDES, "optimizer.max_steps", "20", "log_every_n_step", "5"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=420, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    last = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    save_dir = os.path.join(out, "panonerf_0_1_2")
    assert last["global_step"] == 20 and os.path.samefile(last["save_dir"], save_dir)
    ckpt = torch.load(os.path.join(save_dir, "checkpoints", "last.ckpt"), map_location="cpu", weights_only=False)
    assert ckpt["global_step"] == 20 and ckpt["hyper_parameters"]["optimizer.max_steps"] == 20
    assert os.path.isfile(os.path.join(save_dir, "val_000020", "metrics.json"))
    assert res.stdout.count("[train] step") == 4
