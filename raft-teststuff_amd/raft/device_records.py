"""What the wrappers of a ctypes record array on the device share (DeviceMooring, DeviceArrayMooring,
DeviceRotor): the upload of the records, float64 inputs of a given shape and the per-row record index."""
import numpy as np


class DeviceRecords:
    def __init__(self, device):
        import torch
        self.torch = torch
        self.dev_index = device
        self.device = torch.device(f"cuda:{device}")

    def upload(self, arr):
        """The ctypes record array `arr`, byte for byte, as a uint8 device tensor."""
        raw = np.frombuffer(bytes(arr), dtype=np.uint8).copy()
        return self.torch.tensor(raw, dtype=self.torch.uint8, device=self.device)

    def f64(self, x, shape):
        t = self.torch.as_tensor(np.asarray(x, dtype=float) if not self.torch.is_tensor(x) else x,
                                 dtype=self.torch.float64, device=self.device).contiguous()
        if list(t.shape) != list(shape):
            raise ValueError(f"expected shape {list(shape)}, got {list(t.shape)}")
        return t

    def index(self, idx, n, limit=None, name="sys_idx"):
        """The int32 device tensor of n record indices (None stays None).  With limit, an index outside
        [0, limit) raises ValueError; without, it is passed on as it is and comes back as that row's
        status (7 from the array mooring entries, 3 from rh_rotor_loads)."""
        if idx is None:
            return None
        idx = np.asarray(idx, dtype=np.int32)
        if idx.shape != (n,) or (limit is not None and n and (idx.min() < 0 or idx.max() >= limit)):
            raise ValueError(f"{name}: {n} entries{'' if limit is None else f' in [0, {limit})'} expected")
        return self.torch.tensor(idx, dtype=self.torch.int32, device=self.device)
