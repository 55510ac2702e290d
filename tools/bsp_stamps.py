"""Wall-clock stamps (10 ns ticks) of the paired back-substitution (chol_backsolve_pairs_kernel), per workgroup.
Build: csrc/build.sh -DCHOL_STAMPS -o tools/libs/lib_stamps.so (tools/README.md); STAMPS_LIB selects another file.
Slots: 0 start (wave 0), 1 N tiles formed (wave 0), 2 far tiles summed (wave 0), 3 u solved (wave 4), 4 arrivals seen
(wave 0), 5 after the barrier (wave 6), 6 x_b computed (wave 6), 7 x_b published (wave 6)."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "droid-slam_reserch_amd")]
import numpy as np
import torch

lib = ctypes.CDLL(os.environ.get("STAMPS_LIB", os.path.join(ROOT, "tools", "libs", "lib_stamps.so")))
lib.droid_chol_scratch_doubles.argtypes = [ctypes.c_int]
lib.droid_chol_scratch_doubles.restype = ctypes.c_size_t
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1530
nb = (n + 63) // 64
G = (nb + 1) // 2
rng = np.random.default_rng(0)
A = rng.normal(size=(n, n + 8)); A = A @ A.T + n * 0.1 * np.eye(n); b = rng.normal(size=n)
dA, dbb = torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda()
x = torch.zeros(n, dtype=torch.float64, device="cuda")
scratch = torch.zeros(lib.droid_chol_scratch_doubles(n), dtype=torch.float64, device="cuda")
flag = torch.zeros(1, dtype=torch.int32, device="cuda")
vp = ctypes.c_void_p
lib.droid_chol_solve.argtypes = [vp, vp, vp, ctypes.c_int, vp, vp, vp]
for rep in range(4):
    lib.droid_chol_solve(dA.data_ptr(), dbb.data_ptr(), x.data_ptr(), n, scratch.data_ptr(), flag.data_ptr(), None)
    torch.cuda.synchronize()
    buf = (ctypes.c_ulonglong * (64 * 8))()
    lib.droid_debug_bs_stamps(buf)
    bs = np.array(buf[:], dtype=np.int64).reshape(64, 8)[:G]
    t0 = bs[:, 0].min()
    print(f"solve {rep}: flag {int(flag.item())} err {np.abs(x.cpu().numpy() - np.linalg.solve(A, b)).max():.2e}; "
          f"first start -> last publish {(bs[:, 7].max() - t0) / 100:.2f} us")
print("workgroup: start | N formed | far summed | u solved | arrivals seen | barrier | x_b | published   (us since the first start)")
for J in range(G - 1, -1, -1):
    print(f"J {J:2d}: " + " ".join(f"{(v - t0) / 100:7.2f}" for v in bs[J]))
print("per pair (us): arrivals seen -> barrier | -> x_b | -> published | published -> seen by the next workgroup | hop")
for J in range(G - 2, -1, -1):
    r = bs[J].astype(float) / 100
    up = bs[J + 1].astype(float) / 100
    print(f"J {J:2d}: {r[5]-r[4]:6.2f} {r[6]-r[5]:6.2f} {r[7]-r[6]:6.2f} {r[4]-up[7]:6.2f} {r[7]-up[7]:6.2f}   "
          f"(u solved {r[4]-r[3]:6.2f} us before the arrivals)")
