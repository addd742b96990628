"""Where does a lock-step of K6 (rs_rollout16_kernel, the fused rollout) spend wave 0's cycles?  Diagnostic build with s_memtime
stamps at the phase boundaries of wave 0's loop:

    python -c "from radiation_ppo_amd.build import build; build(defines=['RS_K6_STAMPS'], suffix='_k6stamps')"
    python -c "from radiation_ppo_amd.build import build; build(defines=['RS_K6_STAMPS', 'RS_K6_PARENT_CHAIN'], suffix='_k6stamps_parent')"
    python scripts/k6_stamps.py [N] [obstruction_count]            # RS_STAMPS_LIB selects the library (default: lib/librs_hip_k6stamps.so)

RS_K6_PARENT_CHAIN compiles the chain as it was before the weights, the output layer and the env state left it: the 'before' column.
Read the SHARES, not the run time: every stamp waits for the wave's outstanding LDS and scalar-memory operations, which forbids
overlaps the product kernel has."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["RS_LIB_PATH"] = os.environ.get("RS_STAMPS_LIB") or os.path.join(ROOT, "radiation_ppo_amd", "lib", "librs_hip_k6stamps.so")
import torch  # noqa: E402

from radiation_ppo_amd import _lib  # noqa: E402
from radiation_ppo_amd.envs import RadSearchVec  # noqa: E402
from radiation_ppo_amd.ppo import FusedCollector, VecAgentPPO  # noqa: E402

PH = ["hidden layers", "output layer", "softmax + draw", "buffer stores", "env step", "Welford + mailbox message", "reset",
      "broadcast + barrier"]
N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
OBST = int(sys.argv[2]) if len(sys.argv) > 2 else 0
T, L = 480, 120
torch.manual_seed(0)
env = RadSearchVec(N, number_agents=1, obstruction_count=OBST, enforce_grid_boundaries=OBST != 0, seed=1)
agents = {0: VecAgentPPO(id=0, steps_per_epoch=T, steps_per_episode=L)}
col = FusedCollector(env, agents, T, L)
lib = _lib.load()
lib.rs_debug_k6_stamps.restype = C.c_int
lib.rs_debug_k6_stamps.argtypes = [C.c_void_p, C.c_int]
col.collect()
buf = (C.c_ulonglong * 32)()
lib.rs_debug_k6_stamps(buf, 1)
R = 3
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(R):
    col.collect()
e1.record()
torch.cuda.synchronize()
lib.rs_debug_k6_stamps(buf, 0)
row = 16 * (1 if OBST != 0 else 0)
cyc = [buf[row + q] for q in range(8)]
ticks, steps = buf[row + 14], buf[row + 15]
tot = sum(cyc)
print(f"{os.path.basename(os.environ['RS_LIB_PATH'])}: N = {N}, obstruction_count = {OBST}, {R} launches of {T} lock-steps")
print(f"stamped build: {e0.elapsed_time(e1) / R:.3f} ms per collect() (slower than the product kernel: read the shares)")
print(f"in-kernel clock {tot / max(ticks, 1) * 100:.0f} MHz; {tot / max(steps, 1):.0f} wave-cycles per lock-step (mean over {N // 16} waves)")
for q, c in enumerate(cyc):
    print(f"   {PH[q]:28s} {c / max(steps, 1):8.0f} cyc  {100.0 * c / max(tot, 1):5.1f} %")
