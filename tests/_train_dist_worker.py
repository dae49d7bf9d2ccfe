"""Worker of tests/test_gpu_train.py::test_two_rank_rehearsal (launched by torch.distributed.run, 2 ranks, gloo, both on
cuda:0): Trainer.fit for 5 steps with graph replay requested; the replicas must end bit-identical and rank 0 alone writes.

    _train_dist_worker.py <scene folder> <out dir>
"""
import json
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pano_nerf_amd as pn  # noqa: E402
from pano_nerf_amd import config, train  # noqa: E402

scene_dir, out_dir = sys.argv[1], sys.argv[2]
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
hp = config.finalize(pn.load_config(None, ["train.factor", "1", "train.sample_num", "[0, 1, 2]", "nerf.num_samples", "32",
                                           "train.batch_size", "256", "log_every_n_step", "1"]), out_dir=out_dir)
scene = pn.PanoScene(scene_dir, factor=1, train_views=[0, 1, 2], keep_rotation=False, pano_normals=False, device=dev)

_save = train.Trainer.save


def save(self, path):  # who writes: one marker file per saving rank
    open(os.path.join(out_dir, f"saved_by_rank{self.rank}"), "w").close()
    _save(self, path)


train.Trainer.save = save
tr = train.Trainer(hp, scene, rank=rank, world=world, graph=True)
tr.fit(5)
assert tr.global_step == 5 and len(tr.losses) == 5
mine = tr.model.mlp.flat_params().detach().cpu()
both = [torch.empty_like(mine) for _ in range(world)]
dist.all_gather(both, mine)
assert torch.equal(both[0], both[1]), float((both[0] - both[1]).abs().max())
assert bool(torch.isfinite(mine).all())
loss = torch.tensor([tr.losses[-1][1]], dtype=torch.float64)
losses = [torch.empty_like(loss) for _ in range(world)]
dist.all_gather(losses, loss)
assert float(losses[0]) != float(losses[1])  # every rank drew its own batch
dist.barrier()
with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as fp:  # (two ranks' stdout lines can interleave)
    json.dump({"check": tr.replay_checks, "replaying": tr._graphs.get(True) is not None}, fp)
dist.barrier()
if rank == 0:
    print("TRAIN_DIST_OK", flush=True)
dist.destroy_process_group()
