"""Golden G19 (tests/golden/g19_pointnet2.npz: the reference's own PointNet2MSG on the CPU) against the NumPy
restatements of tests/pointnet2_ref.py and against this package's modules -- no GPU."""
import json
import os

import numpy as np
import pytest

from tests import pointnet2_ref as R


@pytest.fixture(scope="module")
def g19(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g19_pointnet2.npz")))


def meta_of(g):
    return json.loads(bytes(g["meta"]).decode())


def levels(g):
    """[xyz of level 0, 1, ...] of the golden."""
    xyz = g["points"][:, 1:4].reshape(R.G19_B, R.G19_N, 3)
    return [xyz] + [g["sa%d_new_xyz" % k] for k in range(len(R.G19_CFG['SA_CONFIG']['NPOINTS']))]


def test_restatements_reproduce_the_golden_indices_and_distances(g19):
    sa, l_xyz = R.G19_CFG['SA_CONFIG'], levels(g19)
    for k, npoint in enumerate(sa['NPOINTS']):
        ties = []
        idx, new_xyz = R.fps(l_xyz[k], npoint, ties=ties)
        assert not ties                                                    # the tie rule plays no part in G19
        assert np.array_equal(idx, g19["sa%d_fps_idx" % k]) and idx.dtype == np.int32
        assert np.array_equal(new_xyz, g19["sa%d_new_xyz" % k])
        for s, (r, ns) in enumerate(zip(sa['RADIUS'][k], sa['NSAMPLE'][k])):
            ball = R.ball_query(l_xyz[k], new_xyz, r, ns)
            assert np.array_equal(ball, g19["sa%d_ball%d" % (k, s)])
            assert len(np.unique(ball)) > npoint // 2                      # not a degenerate golden
    for k in range(len(R.G19_CFG['FP_MLPS'])):
        dist, idx = R.three_nn(l_xyz[k], l_xyz[k + 1])
        assert np.array_equal(idx, g19["fp%d_nn_idx" % k])
        assert np.array_equal(dist, g19["fp%d_nn_dist" % k]) and dist.dtype == np.float32
    pts = g19["points"]
    assert np.array_equal(g19["point_coords"], pts[:, :4])
    assert g19["point_features"].shape == (R.G19_B * R.G19_N, 16)
    assert meta_of(g19)["thread_deviation"] <= 1e-6


def test_inverse_and_backward_restatements_agree():
    """np.add.at in entry order == the CSR walk of the header (the entries of a source ascending, from +0.0)."""
    rng = np.random.default_rng(7)
    idx = rng.integers(0, 9, 40).astype(np.int32)
    idx[idx == 4] = 5                                                      # a source nobody references
    csr, lst = R.invert(idx, 9)
    assert csr[0] == 0 and csr[-1] == 40 and csr[4] == csr[5]
    g = rng.normal(0, 1, (1, 2, 40)).astype(np.float32)
    want = R.gather_backward(g, idx[None], 9)
    for c in range(2):
        for s in range(9):
            acc = np.float32(0.0)
            for e in lst[csr[s]:csr[s + 1]]:
                assert idx[e] == s
                acc = np.float32(acc + g[0, c, e])
            assert acc == want[0, c, s]
        assert list(lst[csr[5]:csr[6]]) == sorted(lst[csr[5]:csr[6]])


def test_state_dict_keys_equal_the_references_and_g19_loads_strictly(g19):
    import torch
    from dfu3d_amd.pcdet_kitti.pointnet2_backbone import PointNet2MSG
    meta = meta_of(g19)
    small = PointNet2MSG(R.G19_CFG, 3 + R.G19_EXTRA)
    assert list(small.state_dict()) == meta["state_dict_keys"]
    full = PointNet2MSG(R.FULL_CFG, R.FULL_INPUT_CHANNELS)
    assert list(full.state_dict()) == meta["full_state_dict_keys"] and full.num_point_features == 128
    sd = {k: torch.from_numpy(g19["sd_" + k].copy()) for k in meta["state_dict_keys"]}
    res = small.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in small.state_dict().items():
        assert tuple(v.shape) == g19["sd_" + k].shape, k
