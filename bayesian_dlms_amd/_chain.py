"""What the Gibbs drivers (studentt.py, stochvol.py, factorsv.py and, through _dlmfsv.py, dlmfsv.py and dlmfsvsys.py) share about
where a chain lives: its arrays stay on a torch device when an engine or a device tensor is given, and are host arrays otherwise
(injected callables and stub engines, for tests)."""
import numpy as np


def is_torch(a):
    return hasattr(a, "data_ptr")


def host(a):
    return a.detach().cpu().numpy() if is_torch(a) else np.asarray(a)


def or_status(a, b):
    """The per-series status flags of two calls or'ed into one host int32 array (None: a call without status; both: None)."""
    if a is None and b is None:
        return None
    a = 0 if a is None else host(a).astype(np.int32)
    b = 0 if b is None else host(b).astype(np.int32)
    return np.asarray(a | b, dtype=np.int32)


def place(ys, engine, N, T):
    """(put, y): put(a, dtype) moves a host array to where the chain lives -- the device of ys if it is a torch tensor, else the
    engine's, else the host -- and y is ys there as a contiguous float64 [N][T]."""
    torch = dev = None
    if is_torch(ys) or engine is not None:
        import torch
        dev = ys.device if is_torch(ys) else torch.device("cuda", engine.device)

    def put(a, dtype=np.float64):
        a = np.ascontiguousarray(a, dtype=dtype)
        return torch.as_tensor(a, device=dev) if torch is not None else a

    y = ys.reshape(N, T).to(dtype=torch.float64).contiguous() if is_torch(ys) else put(np.asarray(ys, dtype=np.float64).reshape(N, T))
    return put, y
