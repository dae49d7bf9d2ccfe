"""Host-only helpers of pano_nerf_amd.data against the reference's PanoDataset (tests/golden/make_dataset_golden.py ->
dataset_ref.npz): metadata, split, pose conversion, folder-name switches, the downscale rule.  Nothing here touches
pixels: that is the device's work (tests/test_gpu_data.py)."""
import json
import os

import numpy as np
import pytest

from pano_nerf_amd import data

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataset_ref.npz"))


def test_split_lists():
    n = len(GOLD["transform_matrices"])
    train, held = data.split_views(n, list(GOLD["train_views"]))
    assert train == list(GOLD["plain_train_data_list"]) and held == list(GOLD["plain_val_data_list"]) == [1, 4]
    assert data.split_views(4, [3, 0]) == ([3, 0], [1, 2])  # train order kept, held-out ascending
    assert data.split_views(3, None) == ([0, 1, 2], [])
    with pytest.raises(ValueError):
        data.split_views(3, [5])


@pytest.mark.parametrize("folder", ["scene_std_pano", "plain"])
def test_pose_conversion(folder):
    keep, pano = data.name_switches("/some/where/" + folder)
    assert (keep, pano) == ((True, True) if folder == "scene_std_pano" else (False, False))
    for split in ("train", "val"):
        for i, want in zip(GOLD[f"{folder}_{split}_data_list"], GOLD[f"{folder}_{split}_camtoworlds"]):
            got = data.convert_pose(GOLD["transform_matrices"][i], keep)
            assert got.dtype == np.float32 and got.shape == (4, 4)
            assert np.abs(got - want).max() <= 1e-6, (folder, split, i)


def test_name_switches():
    assert data.name_switches("/d/bathroom_rot") == (True, False)
    assert data.name_switches("/d/bathroom_std") == (True, False)
    assert data.name_switches("/d/bathroom_pano") == (False, True)
    assert data.name_switches("/d/bathroom_0") == (False, False)


def test_check_downscale():
    assert data.check_downscale(2048, 4096, 4) == (512, 1024)
    for h, w, f in ((30, 64, 4), (32, 62, 4), (32, 64, 0)):
        with pytest.raises(ValueError):
            data.check_downscale(h, w, f)


def test_read_meta(tmp_path):
    entry = [{"file_path": "a", "transform_matrix": np.eye(4).tolist()}]
    (tmp_path / "transforms_all.json").write_text(json.dumps({"image": entry, "depth": entry}))
    meta = data.read_meta(str(tmp_path))
    assert meta["image"] == entry and meta["depth"] == entry
    assert meta["albedo"] is None and meta["normal"] is None  # a missing material list is reported as absent
    (tmp_path / "other.json").write_text(json.dumps({"albedo": entry}))
    with pytest.raises(ValueError):
        data.read_meta(str(tmp_path), "other")
