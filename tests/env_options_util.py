"""What tests/test_env_options_cpu.py and tests/test_env_options_gpu.py share."""
import torch


def same(a, b):
    """equality of checkpoint records: dicts by keys, tensors by dtype and values, the rest by type and =="""
    if isinstance(a, dict) or isinstance(b, dict):
        return isinstance(a, dict) and isinstance(b, dict) and sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == b.dtype and a.device == b.device and torch.equal(a, b)
    return type(a) is type(b) and a == b
