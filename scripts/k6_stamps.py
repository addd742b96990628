"""Where does a lock-step of K6 (rs_rollout16_kernel, the fused rollout) spend wave 0's cycles?  Diagnostic build with s_memtime
stamps at the phase boundaries of wave 0's loop:

    python -c "from radiation_ppo_amd.build import build; build(defines=['RS_K6_STAMPS'], suffix='_k6stamps')"
    python -c "from radiation_ppo_amd.build import build; build(defines=['RS_K6_STAMPS', 'RS_K6_PARENT_CHAIN'], suffix='_k6stamps_parent')"
    python -c "from radiation_ppo_amd.build import build; build(defines=['RS_K6_STAMPS', 'RS_K6_SERIAL_DRAW'], suffix='_k6stamps_serial')"
    python -c "from radiation_ppo_amd.build import build; build(defines=['RS_K6_STAMPS', 'RS_K6_TILE_WAVES=2'], suffix='_k6stamps_tw2')"
    python -c "from radiation_ppo_amd.build import build; build(defines=['RS_K6_STAMPS', 'RS_K6_TILE_WAVES=0'], suffix='_k6stamps_tw0')"
    python scripts/k6_stamps.py [N] [obstruction_count]            # RS_STAMPS_LIB selects the library (default: lib/librs_hip_k6stamps.so)

RS_K6_PARENT_CHAIN compiles the chain as it was before the weights, the output layer and the env state left it: the 'before' column.
RS_K6_SERIAL_DRAW compiles the serial measurement draw (rs_poisson) and the action draw's own Philox call inside the softmax: the
'before' column of the grouped draw.  RS_K6_TILE_WAVES=2 / =0 compile the actor's hidden layers on two tile waves / in wave 0 alone
(the 'before' column of the tile waves); with tile waves "hidden layers" includes wave 0's waits at the two exchanges, shown below it.  Below the phase table: the measurement draw's cycles inside "env step", the trips of the
serial loop per lock-step (the candidates the wave's slowest env needs) and the cycles of the action draw's Philox call.
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
NPH = 20                                    # RS_K6_NPH
buf = (C.c_ulonglong * (2 * NPH))()
lib.rs_debug_k6_stamps(buf, 1)
R = 3
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(R):
    col.collect()
e1.record()
torch.cuda.synchronize()
lib.rs_debug_k6_stamps(buf, 0)
row = NPH * (1 if OBST != 0 else 0)
cyc = [buf[row + q] for q in range(8)]
xch = [buf[row + 16], buf[row + 17]]       # tile waves: from wave 0's tile store to the exchanged tiles read back (barrier included)
cyc[0] += sum(xch)
cyc[4] -= buf[row + 11]                     # counting the candidates is the diagnostic's own work inside "env step"
if buf[row + 13]:
    PH.append("draw blocks (one Philox call)")
    cyc.append(buf[row + 13])
ticks, steps = buf[row + 14], buf[row + 15]
tot = sum(cyc)
print(f"{os.path.basename(os.environ['RS_LIB_PATH'])}: N = {N}, obstruction_count = {OBST}, {R} launches of {T} lock-steps")
print(f"stamped build: {e0.elapsed_time(e1) / R:.3f} ms per collect() (slower than the product kernel: read the shares)")
print(f"in-kernel clock {tot / max(ticks, 1) * 100:.0f} MHz; {tot / max(steps, 1):.0f} wave-cycles per lock-step (mean over {N // 16} waves)")
for q, c in enumerate(cyc):
    print(f"   {PH[q]:28s} {c / max(steps, 1):8.0f} cyc  {100.0 * c / max(tot, 1):5.1f} %")
if sum(xch):
    print(f"   inside hidden layers: H1 exchange {xch[0] / max(steps, 1):.0f} cyc, H2 exchange {xch[1] / max(steps, 1):.0f} cyc (barrier, wait for the slowest tile wave, loads)")
poi, trips, left, phx = (buf[row + q] / max(steps, 1) for q in (8, 9, 10, 12))
print(f"   inside env step: measurement draw {poi:.0f} cyc ({100.0 * poi * steps / max(tot, 1):.1f} %); a serial loop needs {trips:.3f} trips per lock-step, "
      f"{left:.3f} of them beyond candidate 3; Philox call of the action draw {phx:.0f} cyc")
if not buf[row + 13]:
    print(f"   predicted saving of the grouped draw: (trips - 1) / trips x draw + 2 Philox calls = {(trips - 1) / max(trips, 1e-9) * poi + 2 * phx:.0f} cyc "
          f"= {100.0 * ((trips - 1) / max(trips, 1e-9) * poi + 2 * phx) * steps / max(tot, 1):.1f} % of the lock-step")
