"""The pieces of pcdet/utils/common_utils.py the anchor head needs, under its names: `limit_period`; and `cfg_get`, the one
way the anchor modules read a configuration that may be the reference's EasyDict, a plain dict or an object."""
import numpy as np
import torch


def cfg_get(cfg, key, *default):
    """cfg[key] / cfg.key; with a default, that when the key is absent."""
    if isinstance(cfg, dict):
        return cfg[key] if not default else cfg.get(key, default[0])
    return getattr(cfg, key) if not default else getattr(cfg, key, default[0])


def limit_period(val, offset=0.5, period=np.pi):
    """val - floor(val / period + offset) * period, in the dtype of val (a NumPy array goes through torch and back)."""
    is_numpy = isinstance(val, np.ndarray)
    if is_numpy:
        val = torch.from_numpy(val).float()
    ans = val - torch.floor(val / period + offset) * period
    return ans.numpy() if is_numpy else ans
