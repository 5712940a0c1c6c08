"""CPU tests of the runner's host half (nice_slam_amd/slam.py): ``load_config`` against what the reference's own loader made of
five of its settings files (tests/golden/configs/, minted by tests/golden/make_golden_config.py), the pretrained-decoder
filter of src/NICE_SLAM.py:159-190, the camera update, and the trajectory error against tools/ate.py."""
import copy
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from nice_slam_amd import NICE
from nice_slam_amd import slam as S

CONFIGS = os.path.join(GOLDEN, "configs")


@pytest.fixture(scope="module")
def merged():
    return json.load(open(os.path.join(CONFIGS, "merged.json")))


@pytest.mark.parametrize("name", ["nice_slam", "replica", "room0", "tum", "freiburg1_desk", "room0_no_default"])
def test_load_config_equals_the_reference(merged, name):
    rec = merged[name]
    default = None if rec["default"] is None else os.path.join(CONFIGS, rec["default"])
    cfg = S.load_config(os.path.join(CONFIGS, rec["config"]), default)
    assert cfg == rec["cfg"]
    assert json.loads(json.dumps(cfg)) == rec["cfg"]
    if name == "room0":                                        # the chain: scene over dataset over the default file
        assert cfg["inherit_from"] == "configs/Replica/replica.yaml" and cfg["dataset"] == "replica"
        assert cfg["mapping"]["bound"][0] == [-2.9, 8.9] and cfg["mapping"]["iters"] == 60 and cfg["tracking"]["lr"] == 0.001
    if name == "freiburg1_desk":
        assert cfg["tracking"]["seperate_LR"] is True and cfg["cam"]["crop_edge"] == 8 and cfg["mapping"]["every_frame"] == 1


def test_load_config_from_the_chain_root_and_update_recursive(merged, monkeypatch, tmp_path):
    monkeypatch.chdir(GOLDEN)                                  # where 'configs/...' resolves as written, like the reference's root
    assert S.load_config("configs/Replica/room0.yaml", "configs/nice_slam.yaml") == merged["room0"]["cfg"]
    a = {"x": {"y": 1, "z": 2}, "k": 3}
    S.update_recursive(a, {"x": {"y": 5, "w": {"v": 1}}, "n": [1, 2]})
    assert a == {"x": {"y": 5, "z": 2, "w": {"v": 1}}, "k": 3, "n": [1, 2]}
    with pytest.raises(FileNotFoundError):
        S.load_config(str(tmp_path / "missing.yaml"))


def _reference_checkpoints(src: NICE):
    """the two ConvONet checkpoints with the reference's prefixes (NICE_SLAM.py:166-190), plus encoder weights to be skipped"""
    coarse = {"decoder." + k: v.clone() for k, v in src.coarse_decoder.state_dict().items()}
    coarse["encoder.fc_pos.weight"] = torch.ones(3, 3)
    coarse["encoder_decoder_note"] = torch.zeros(1)                       # 'decoder' AND 'encoder' in the key: skipped
    mf = {"decoder.coarse." + k: v.clone() for k, v in src.middle_decoder.state_dict().items()}
    mf.update({"decoder.fine." + k: v.clone() for k, v in src.fine_decoder.state_dict().items()})
    mf["encoder.unet3d.encoders.0.weight"] = torch.ones(2, 2)
    mf["encoder.fine.decoder_like"] = torch.zeros(1)
    return {"model": coarse}, {"model": mf}


def test_pretrained_decoders_are_filtered_and_stripped(tmp_path):
    torch.manual_seed(3)
    src, dst = NICE(coarse=True), NICE(coarse=True)
    before = {k: v.clone() for k, v in dst.state_dict().items()}
    ck_c, ck_mf = _reference_checkpoints(src)
    torch.save(ck_c, tmp_path / "coarse.pt")
    torch.save(ck_mf, tmp_path / "middle_fine.pt")
    cfg = {"coarse": True, "pretrained_decoders": {"coarse": str(tmp_path / "coarse.pt"), "middle_fine": str(tmp_path / "middle_fine.pt")}}
    S.load_pretrained(dst, cfg)
    want, got = src.state_dict(), dst.state_dict()
    assert list(want) == list(got)
    for k in want:
        if k.startswith("color_decoder."):                    # not part of the pretrained checkpoints: left as initialised
            assert torch.equal(got[k], before[k]), k
        else:
            assert torch.equal(got[k], want[k]), k
    assert not torch.equal(got["middle_decoder.pts_linears.0.weight"], before["middle_decoder.pts_linears.0.weight"])
    # without the coarse level only middle_fine is read
    dst2 = NICE(coarse=False)
    S.load_pretrained(dst2, {"coarse": False, "pretrained_decoders": {"coarse": str(tmp_path / "nowhere.pt"), "middle_fine": str(tmp_path / "middle_fine.pt")}})
    assert all(torch.equal(dst2.state_dict()[k], want[k]) for k in dst2.state_dict() if not k.startswith("color_decoder."))


def test_missing_pretrained_checkpoint_names_the_path(tmp_path, merged):
    path = str(tmp_path / "pretrained" / "coarse.pt")
    cfg = {"coarse": True, "pretrained_decoders": {"coarse": path, "middle_fine": path}}
    with pytest.raises(FileNotFoundError) as e:
        S.load_pretrained(NICE(coarse=True), cfg)
    assert path in str(e.value)


def test_imap_is_refused_like_the_renderer(merged, tmp_path):
    cfg = copy.deepcopy(merged["room0"]["cfg"])
    args = types.SimpleNamespace(input_folder=None, output=str(tmp_path / "out"), nice=False)
    with pytest.raises(NotImplementedError) as e:
        S.NICE_SLAM(cfg, args, decoders="random")
    assert "iMAP" in str(e.value)
    assert not os.path.exists(tmp_path / "out")                # refused before anything is created


def test_update_cam_crop_size_then_crop_edge(merged):
    slam = S.NICE_SLAM.__new__(S.NICE_SLAM)
    slam.cfg = merged["freiburg1_desk"]["cfg"]
    cam = slam.cfg["cam"]
    slam.H, slam.W, slam.fx, slam.fy, slam.cx, slam.cy = (cam[k] for k in ("H", "W", "fx", "fy", "cx", "cy"))
    slam.update_cam()
    sx, sy = 512 / 640, 384 / 480                             # NICE_SLAM.py:119-135
    assert (slam.H, slam.W) == (384 - 16, 512 - 16)
    assert (slam.fx, slam.fy, slam.cx, slam.cy) == (sx * 517.3, sy * 516.5, sx * 318.6 - 8, sy * 255.3 - 8)


def test_ate_equals_the_tools_formula():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ate
    rng = np.random.RandomState(2)
    gt = np.tile(np.eye(4), (30, 1, 1))
    gt[:, :3, 3] = np.cumsum(rng.randn(30, 3) * 0.05, 0)
    est = gt.copy()
    est[:, :3, 3] = gt[:, :3, 3] @ np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]) + 0.3 + rng.randn(30, 3) * 0.01
    assert S.ate_rmse(list(est), list(gt)) == ate.ate_rmse(list(est), list(gt))
    assert 0.0 < S.ate_rmse(list(est), list(gt))["rmse"] < 0.03


def test_checkpoint_keys_are_the_loggers():
    assert S.CKPT_KEYS == ("c", "decoder_state_dict", "gt_c2w_list", "estimate_c2w_list", "keyframe_list", "selected_keyframes", "idx")
