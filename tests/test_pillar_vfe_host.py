"""The pillar feature encoder without a GPU: the C ABI of include/dfu3d_vfe.h, host-side argument validation, the
modules' state-dict keys, and the numpy restatement (tests/pillar_vfe_ref.py) against golden G13."""
import ctypes
import json
import os

import numpy as np
import pytest

from dfu3d_amd import _lib, _lib_vfe
from tests import pillar_vfe_ref as R

P16 = ctypes.c_void_p(16)            # a non-null, 16-byte aligned address no call may touch


@pytest.fixture(scope="module")
def g13(golden_dir):
    g = np.load(os.path.join(golden_dir, "g13_pillar_vfe.npz"))
    return g, json.loads(bytes(g["meta"]).decode())


def test_library_exports_every_symbol_of_the_vfe_header():
    L = _lib_vfe.lib()
    assert _lib_vfe.header_symbols() == sorted([
        "dfu3d_vfe_version", "dfu3d_vfe_scratch_bytes", "dfu3d_pillar_group", "dfu3d_pillar_features",
        "dfu3d_pillar_max", "dfu3d_pillar_max_backward"])
    for name in _lib_vfe.header_symbols():
        assert getattr(L, name).argtypes is not None
    assert L.dfu3d_vfe_version() == _lib_vfe.header_version() == 100
    assert not set(_lib_vfe.SIGNATURES) & set(_lib.SIGNATURES)
    assert all(k.startswith("DFU3D_VFE_") for k in _lib_vfe.CONSTANTS)


def test_binding_names_a_missing_symbol():
    class Fake:
        _name = "fake.so"
        dfu3d_vfe_version = dfu3d_pillar_group = dfu3d_pillar_features = dfu3d_pillar_max = object()
    with pytest.raises(_lib.Dfu3dError, match="dfu3d_pillar_max_backward, dfu3d_vfe_scratch_bytes"):
        _lib_vfe.bind(Fake())


def _group(L, points=P16, n=8, cols=5, B=1, nx=4, ny=4, first_out=P16, scratch=P16, nbytes=1 << 20):
    return L.dfu3d_pillar_group(points, n, cols, B, 0.0, 0.0, 1.0, 1.0, nx, ny, 0, first_out, P16, P16, P16, P16, P16, P16,
                                P16, scratch, nbytes, None)


def test_bad_arguments_return_before_any_launch():
    L = _lib_vfe.lib()
    K = _lib.CONSTANTS
    EINVAL, ERANGE = K["DFU3D_EINVAL"], K["DFU3D_ERANGE"]
    V = _lib_vfe.CONSTANTS
    assert _group(L, points=None) == EINVAL
    assert _group(L, first_out=None) == EINVAL
    assert _group(L, scratch=None) == EINVAL
    assert _group(L, cols=3) == EINVAL
    assert _group(L, nbytes=8) == EINVAL                                             # scratch too small
    assert _group(L, B=2, nx=4096, ny=4096) == ERANGE                                  # more cells than MAX_CELLS
    assert _group(L, B=1, nx=V["DFU3D_VFE_MAX_CELLS"] + 1, ny=1) == ERANGE
    assert L.dfu3d_vfe_scratch_bytes(10, V["DFU3D_VFE_MAX_CELLS"] + 1) == -1
    assert L.dfu3d_vfe_scratch_bytes(-1, 10) == -1
    assert L.dfu3d_vfe_scratch_bytes(1000, 4096) >= 3 * 4000 + 2 * 512
    assert L.dfu3d_pillar_features(None, 8, 5, 0.0, 0.0, 1.0, 1.0, 0.5, 0.5, 0.5, 0, 1, 0, P16, P16, P16, P16, P16, P16, 10,
                                   P16, 1 << 20, None) == EINVAL
    assert L.dfu3d_pillar_features(P16, 8, 5, 0.0, 0.0, 1.0, 1.0, 0.5, 0.5, 0.5, 0, 1, 0, P16, P16, P16, P16, P16, P16, 11,
                                   P16, 1 << 20, None) == EINVAL                       # width of the layout is 10
    assert L.dfu3d_pillar_max(P16, 8, V["DFU3D_VFE_MAX_CHANNELS"] + 1, P16, P16, 4, P16, P16, P16, None, None) == ERANGE
    assert L.dfu3d_pillar_max(None, 8, 32, P16, P16, 4, P16, P16, P16, None, None) == EINVAL
    assert L.dfu3d_pillar_max(P16, 8, 32, P16, P16, 4, None, P16, P16, None, None) == EINVAL
    assert L.dfu3d_pillar_max_backward(None, None, 8, 32, P16, P16, P16, 4, P16, P16, None) == EINVAL
    assert L.dfu3d_pillar_max_backward(P16, P16, 8, 32, P16, P16, P16, 4, P16, P16, None) == EINVAL
    assert L.dfu3d_pillar_max_backward(P16, None, 8, 257, P16, P16, P16, 4, P16, P16, None) == ERANGE
    assert L.dfu3d_pillar_max_backward(P16, None, 8, 32, P16, P16, P16, 4, P16, None, None) == EINVAL


def test_modules_build_without_a_gpu_with_the_reference_state_dict_keys(g13):
    from dfu3d_amd.pcdet_kitti import dynamic_pillar_vfe as M
    g, meta = g13
    for name, cfg in R.CFGS.items():
        for model_cfg in (cfg['model_cfg'], type('Cfg', (), cfg['model_cfg'])):     # dict and attribute access
            vfe = getattr(M, cfg['cls'])(model_cfg=model_cfg, num_point_features=cfg['num_point_features'],
                                         voxel_size=cfg['voxel_size'], grid_size=cfg['grid_size'],
                                         point_cloud_range=cfg['point_cloud_range'])
            sd = vfe.state_dict()
            assert list(sd) == meta[name + '_state_dict_keys']
            for k, v in sd.items():
                assert tuple(v.shape) == g['%s_sd_%s' % (name, k)].shape and v.device.type == 'cpu', k
            assert vfe.get_output_feature_dim() == cfg['model_cfg']['NUM_FILTERS'][-1]
            assert all(not hasattr(v, 'device') for v in vars(vfe).values())          # geometry kept as Python numbers
    layer = M.PFNLayerV2(10, 64, use_norm=True, last_layer=False)
    assert layer.linear.weight.shape == (32, 10) and layer.norm.eps == 1e-3 and layer.norm.momentum == 0.01


@pytest.mark.parametrize("name", sorted(R.CFGS))
def test_ref_restatement_reproduces_g13_exactly(g13, name):
    g, _ = g13
    cfg = R.CFGS[name]
    m = cfg['model_cfg']
    pts = g[name + '_points']
    gr = R.group(pts, cfg['batch_size'], cfg['point_cloud_range'], cfg['voxel_size'], cfg['grid_size'], cfg['layout'])
    assert gr['status'] == 0 and 0 < len(gr['kept_idx']) < len(pts)
    for k in ('unq_inv', 'unq_cnt', 'coords'):
        assert gr[k].dtype == g[name + '_' + k].dtype and np.array_equal(gr[k], g[name + '_' + k]), k
    f = R.features(pts, gr, cfg['point_cloud_range'], cfg['voxel_size'], R.offsets_of(cfg), cfg['layout'],
                   m['USE_ABSLOTE_XYZ'], m['WITH_DISTANCE'])
    assert f.dtype == np.float32 and np.array_equal(f, g[name + '_features_in'])
    P = len(gr['unq_cnt'])
    for i in range(len(m['NUM_FILTERS'])):
        x = g['%s_l%d_x' % (name, i)]
        x_max, arg = R.pillar_max(x, gr['unq_inv'], P)
        assert np.array_equal(x_max, g['%s_l%d_x_max' % (name, i)])
        assert np.array_equal(x[arg, np.arange(x.shape[1])[None, :]], x_max)
        assert (gr['unq_inv'][arg] == np.arange(P)[:, None]).all()
    assert np.array_equal(g[name + '_final_eval'], g['%s_l%d_x_max' % (name, len(m['NUM_FILTERS']) - 1)])


def test_ref_backward_matches_torch_autograd_on_the_cpu(g13):
    """The written-out backward of the two scatter functions against autograd of the torch composition (float64, where
    the order of a sum does not show at this size)."""
    import torch
    rng = np.random.default_rng(5)
    inv = np.sort(rng.integers(7, size=40)).astype(np.int64)
    rng.shuffle(inv)
    inv = np.unique(inv, return_inverse=True)[1].reshape(-1)
    P = int(inv.max()) + 1
    x = rng.integers(0, 3, size=(40, 5)).astype(np.float32)                          # many ties
    _, arg = R.pillar_max(x, inv, P)
    gc = rng.integers(-4, 5, size=(40, 10)).astype(np.float32)                       # small integers: every sum is exact
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    it = torch.from_numpy(inv)
    x_max = torch.zeros(P, 5, dtype=torch.float64).scatter_reduce(0, it.view(-1, 1).expand(-1, 5), xt, 'amax', include_self=False)
    assert np.array_equal(x_max.detach().numpy(), R.pillar_max(x, inv, P)[0])
    # autograd of amax splits a gradient evenly among ties; route by the arg instead, as torch_scatter does
    picked = xt[torch.from_numpy(arg.astype(np.int64)), torch.arange(5)[None, :]]
    torch.cat([xt, picked[it]], 1).backward(torch.from_numpy(gc).double())
    assert np.array_equal(xt.grad.numpy().astype(np.float32), R.pillar_max_concat_backward(gc, arg, inv))
    gm = rng.integers(-4, 5, size=(P, 5)).astype(np.float32)
    xt.grad = None
    xt[torch.from_numpy(arg.astype(np.int64)), torch.arange(5)[None, :]].backward(torch.from_numpy(gm).double())
    assert np.array_equal(xt.grad.numpy().astype(np.float32), R.pillar_max_backward(gm, arg, 40))
