"""How far apart do the two waves of a SIMD leave K7's trip loop, and how long do the waves then wait at the epilogue's first barrier?
Diagnostic build without phase stamps (python radiation_ppo_amd/build.py --skew [--prio N] -> lib/librs_hip_skew[_prioN].so, selected
through RS_SKEW_LIB or RS_LIB_PATH): three s_memtime reads per wave and launch, none inside the loop, so the trips overlap as in the
product build (rs_ppo_grad2.hpp, RS_K7_SKEW).  Prints, per network:
  - the mean loop-end time of every wave slot and its mean wait at the barrier,
  - on which SIMD the waves of a slot ran (HW_ID), i.e. which slots are partners,
  - for the pairs (w, w + 4) the mean of loop-end(w + 4) - loop-end(w), signed and absolute, in us, in paired trips (kernel time /
    trips) and in solo trips (the same kernel with RS_K7_THREADS=256, one wave per SIMD, measured in a child process of its own).

    python scripts/k7_partner_gap.py [M]        # M defaults to 4096 x 480 = 1 966 080
"""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["RS_LIB_PATH"] = os.environ.get("RS_SKEW_LIB") or os.environ.get("RS_LIB_PATH") or os.path.join(
    ROOT, "radiation_ppo_amd", "lib", "librs_hip_skew.so")
M = int(sys.argv[1]) if len(sys.argv) > 1 else 4096 * 480
SOLO = os.environ.get("RS_K7_THREADS") == "256"
NSK, R = 66, 10
NETS = ((0, "actor"), (1, "critic"))


def solo_trips():
    """{network: us per trip of a wave that has its SIMD to itself}: this script once more, as a child with RS_K7_THREADS=256"""
    env = dict(os.environ, RS_K7_THREADS="256")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), str(M)], env=env, capture_output=True, text=True, timeout=240)
    if out.returncode != 0:
        raise RuntimeError(f"solo run failed ({out.returncode}):\n{out.stdout}\n{out.stderr}")
    got = {}
    for line in out.stdout.splitlines():
        if line.startswith("SOLO "):
            _, name, us = line.split()
            got[name] = float(us)
    return got


def measure():
    import torch
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.ppo import FFActorCritic, FusedPPOGrad
    torch.manual_seed(0)
    ac = FFActorCritic().cuda()
    X = torch.randn(M, 11, device="cuda")
    act = torch.randint(0, 8, (M,), device="cuda")
    adv, ret, lpo = torch.randn(M, device="cuda"), torch.randn(M, device="cuda"), -2.0 + 0.1 * torch.randn(M, device="cuda")
    w = torch.full((M,), 1.0 / M, device="cuda")
    f = FusedPPOGrad(ac)
    lib = _lib.load()
    lib.rs_debug_k7_skew.restype = C.c_int
    lib.rs_debug_k7_skew.argtypes = [C.c_void_p, C.c_int]
    for _ in range(3):
        f(X, act, adv, ret, lpo, w, 0.2, 0.1)
    buf = (C.c_ulonglong * (2 * NSK))()
    assert lib.rs_debug_k7_skew(buf, 1) == 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(R):
        f(X, act, adv, ret, lpo, w, 0.2, 0.1)
    e1.record()
    torch.cuda.synchronize()
    assert lib.rs_debug_k7_skew(buf, 0) == 0
    return e0.elapsed_time(e1) / R, [[buf[n * NSK + q] for q in range(NSK)] for n in range(2)]


def signed(v):
    return v - (1 << 64) if v >= (1 << 63) else v


def main():
    solo = None if SOLO else solo_trips()
    ms, tab = measure()
    slots = 4 if SOLO else 8
    trips = -(-((M + 31) // 32) // 2048)
    if not SOLO:
        print(f"{os.path.basename(os.environ['RS_LIB_PATH'])}: M = {M}, {trips} trips per wave, {ms:.3f} ms per rs_ppo_grad (both networks + reduce)")
    for net, name in NETS:
        T = tab[net]
        launches = T[64]
        per_slot = sum(T[24:28])                       # waves of slot 0 seen on any SIMD = workgroups x launches
        assert launches == R and per_slot % launches == 0, (launches, per_slot)
        mhz = sum(T[16:16 + slots]) / max(T[65], 1) * 100.0
        us = lambda cyc, n=per_slot: cyc / n / mhz     # noqa: E731
        kern = sum(us(T[16 + w]) for w in range(slots)) / slots
        if SOLO:
            print(f"SOLO {name} {kern / trips:.4f}")
            continue
        paired = kern / trips
        print(f"{name}: in-kernel clock {mhz:.0f} MHz, {per_slot // launches} workgroups, kernel end {kern:.1f} us -> one paired trip {paired:.2f} us, "
              f"one solo trip {solo[name]:.2f} us (a lone wave does a trip in {solo[name] / paired:.2f} paired trips)")
        print("   slot   loop end us   barrier wait us   epilogue us   SIMD 0..3 (share of the slot's waves)")
        for w in range(8):
            hist = T[24 + 4 * w:28 + 4 * w]
            print(f"   {w:4d} {us(T[w]):13.1f} {us(T[8 + w] - T[w]):17.1f} {us(T[16 + w] - T[8 + w]):13.1f}   "
                  + " ".join(f"{h / per_slot:5.2f}" for h in hist))
        same = [sum(min(T[24 + 4 * w + s], T[24 + 4 * (w + 4) + s]) for s in range(4)) / per_slot for w in range(4)]
        print("   slots w and w + 4 on the same SIMD (upper bound from the two histograms): " + " ".join(f"{v:.2f}" for v in same))
        gaps, absg = [], []
        for w in range(4):
            g, a = us(signed(T[56 + w])), us(T[60 + w])
            gaps.append(g)
            absg.append(a)
            print(f"   pair ({w}, {w + 4}): loop end {w + 4} - loop end {w} = {g:8.1f} us = {g / paired:6.2f} paired = {g / solo[name]:6.2f} solo trips;"
                  f"  |.| {a:7.1f} us, sign consistency {abs(g) / max(a, 1e-9):.2f}")
        wait = sum(us(T[8 + w] - T[w]) for w in range(8)) / 8
        mg = sum(gaps) / 4
        print(f"   {name} mean partner gap {mg:.1f} us = {mg / paired:.2f} paired trips (mean |gap| {sum(absg) / 4:.1f} us = {sum(absg) / 4 / paired:.2f});"
              f" mean wait at the barrier {wait:.1f} us")


if __name__ == "__main__":
    main()
