"""Checkpoint mapping of pano_nerf_amd.train without a device: a dict in the layout of the reference's Lightning
checkpoints (state_dict under mip_nerf.mlp.*, optimizer_states[0] = torch.optim.Adam.state_dict(), global_step) maps to
the flat parameter / moment vectors entry for entry, and the package's own checkpoint dict round-trips through
torch.save / torch.load."""
import torch

from pano_nerf_amd import train
from pano_nerf_amd.mlp import RadianceMLP


def _trained_copy(nc, steps=3):
    torch.manual_seed(7)
    mlp = RadianceMLP(num_density_channels=nc)
    opt = torch.optim.Adam(mlp.parameters(), lr=2e-4)
    for s in range(steps):
        opt.zero_grad()
        for i, p in enumerate(mlp.parameters()):
            p.grad = torch.randn_like(p) * (1.0 + i)
        opt.step()
    return mlp, opt


def _expected(mlp, opt):
    """Flat vectors built straight from Adam's per-parameter state, in mlp.parameters() order, at the block's offsets."""
    flat, m, v = (torch.zeros(mlp._total) for _ in range(3))
    for (k, p) in mlp.named_parameters():
        o = mlp._offsets[k]
        st = opt.state[p]
        flat[o:o + p.numel()] = p.detach().reshape(-1)
        m[o:o + p.numel()] = st["exp_avg"].reshape(-1)
        v[o:o + p.numel()] = st["exp_avg_sq"].reshape(-1)
    return flat, m, v


def test_lightning_layout_maps_to_flat_state():
    for nc in (5, 1):
        mlp, opt = _trained_copy(nc)
        ckpt = {"state_dict": {"mip_nerf.mlp." + k: v.clone() for k, v in mlp.state_dict().items()},
                "optimizer_states": [opt.state_dict()], "global_step": 3, "epoch": 0, "lr_schedulers": [{}]}
        fresh = RadianceMLP(num_density_channels=nc)
        flat, m, v, step, gstep = train.flat_state_from_checkpoint(ckpt, fresh)
        want = _expected(mlp, opt)
        assert (step, gstep) == (3, 3)
        assert flat.shape == (mlp._total,) and float(m.abs().max()) > 0 and float(v.max()) > 0
        for got, w in zip((flat, m, v), want):
            assert torch.equal(got, w)
        # the concatenation of Adam's per-parameter state in mlp.parameters() order = the flat vector's occupied entries
        cat = torch.cat([opt.state[p]["exp_avg"].reshape(-1) for p in mlp.parameters()])
        occupied = torch.cat([m[mlp._offsets[k]:mlp._offsets[k] + p.numel()] for k, p in mlp.named_parameters()])
        assert torch.equal(cat, occupied)


def test_own_checkpoint_round_trip(tmp_path):
    mlp, opt = _trained_copy(5)
    flat, m, v = _expected(mlp, opt)
    rng = {"cpu": torch.get_rng_state(), "cuda": torch.zeros(16, dtype=torch.uint8)}
    ckpt = train.checkpoint_dict(mlp, m, v, 3, 12, {"seed": 4, "train.sample_num": [0, 2], "checkpoint.resume_path": None},
                                 lr=2e-4, rng=rng)
    assert set(ckpt["state_dict"]) == {"mip_nerf.mlp." + k for k in mlp.state_dict()}
    assert "mip_nerf.mlp.layers.0.0.weight" in ckpt["state_dict"] and "mip_nerf.mlp.color_layer.bias" in ckpt["state_dict"]
    path = str(tmp_path / "last.ckpt")
    torch.save(ckpt, path)
    back = torch.load(path, map_location="cpu", weights_only=False)
    assert back["global_step"] == 12 and back["hyper_parameters"]["train.sample_num"] == [0, 2]
    assert torch.equal(back["rng_states"]["cpu"], rng["cpu"])
    f2, m2, v2, step, gstep = train.flat_state_from_checkpoint(back, RadianceMLP(num_density_channels=5))
    assert (step, gstep) == (3, 12)
    assert torch.equal(f2, flat) and torch.equal(m2, m) and torch.equal(v2, v)
    # the optimizer part is what torch.optim.Adam itself loads
    again = torch.optim.Adam(RadianceMLP(num_density_channels=5).parameters(), lr=1.0)
    again.load_state_dict(back["optimizer_states"][0])
    assert again.param_groups[0]["lr"] == 2e-4


def test_before_the_first_step_there_is_no_adam_state():
    mlp = RadianceMLP(num_density_channels=5)
    z = torch.zeros(mlp._total)
    ckpt = train.checkpoint_dict(mlp, z, z, 0, 0)
    flat, m, v, step, gstep = train.flat_state_from_checkpoint(ckpt, mlp)
    assert (step, gstep) == (0, 0) and not m.any() and not v.any() and torch.equal(flat, _expected_params(mlp))


def _expected_params(mlp):
    flat = torch.zeros(mlp._total)
    for k, p in mlp.named_parameters():
        flat[mlp._offsets[k]:mlp._offsets[k] + p.numel()] = p.detach().reshape(-1)
    return flat
