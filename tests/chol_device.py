"""The one way the accuracy tests call droid_chol_solve (tests/test_gpu_chol_accuracy.py and the child processes it starts)."""
import numpy as np


def solve(lib, torch, A, b, scratch=None):
    """One droid_chol_solve with x preset to NaN and a zeroed scratch unless one is handed in.
    Returns (rc, flag, x as numpy, scratch)."""
    n = len(b)
    dA = torch.from_numpy(np.ascontiguousarray(A, dtype=np.float64)).cuda()
    db = torch.from_numpy(np.ascontiguousarray(b, dtype=np.float64)).cuda()
    x = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    if scratch is None:
        scratch = torch.zeros(lib.droid_chol_scratch_doubles(n), dtype=torch.float64, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = lib.droid_chol_solve(dA.data_ptr(), db.data_ptr(), x.data_ptr(), n, scratch.data_ptr(), flag.data_ptr(),
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, int(flag.item()), x.cpu().numpy(), scratch
