#!/usr/bin/env python3
"""How much of the Dice bound the INPUTS of tests/test_loop_parity_gpu.py use up, on the CPU oracle alone (no device).

  python3 tools/loop_parity_floor.py [a] [b] [c] [weights=<seed>] [inputs=<seed>]

For each case (tests/loop_parity_cases.py) it prints, of the oracle's result (a, c: the sum of the x0 predictions; b: x_0):
  * the per-class share of voxels the binarisation keeps (the test asserts 2 % .. 98 % for every class);
  * the share of voxels within 0.01 of the threshold;
  * the fp16-input floor: 1 - min Dice between the oracle and the same oracle whose model x input alone is rounded through
    fp16 on the steps the product runs on fp16 operands (a, c: every step; b: model timesteps >= 2, the last two steps run on
    the fp32 companion plan).  The test wants it at most 2.5e-4, a quarter of the bound, so that a red Dice assertion
    is the kernels' doing and not the draw's.
``weights=`` / ``inputs=`` replace the case's seeds (choosing them); DESIGN 2 keeps the output for the seeds in use."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FLOOR_MAX = 2.5e-4


def report(name, want, rounded, seconds):
    import loop_parity_cases as L
    from oracle.unet_ref import binarise
    sh = L.shares(binarise(want))
    near = float((want.abs() < 0.01).float().mean())
    fl = L.floor(want, rounded)
    d = (want - rounded).abs()
    ok = L.SHARE_MIN < min(sh) and max(sh) < L.SHARE_MAX and fl <= FLOOR_MAX
    print(f"case {name}: shares min {min(sh):.4f} max {max(sh):.4f} [{' '.join(f'{s:.3f}' for s in sh)}]")
    print(f"case {name}: |value| < 0.01 on {100 * near:.3f} % of the voxels; fp16-input floor {fl:.2e} "
          f"(|d| max {d.max():.2e} mean {d.mean():.2e}); {'suitable' if ok else 'UNSUITABLE'}; oracle {seconds:.0f} s", flush=True)
    return ok


def main(argv):
    import torch
    import loop_parity_cases as L
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    cases = [a for a in argv if a in ("a", "b", "c")] or ["a", "b", "c"]
    opts = dict(a.split("=") for a in argv if "=" in a)
    ok = True
    if "a" in cases or "b" in cases:
        L.SEED_WEIGHTS_UNET = int(opts.get("weights", L.SEED_WEIGHTS_UNET))
        _, ref = L.unet_nets()
        if "a" in cases:
            L.SEED_INPUTS_A = int(opts.get("inputs", L.SEED_INPUTS_A))
            inp, t0 = L.inputs_a(), time.time()
            ok &= report(f"a (weights {L.SEED_WEIGHTS_UNET}, inputs {L.SEED_INPUTS_A})", L.oracle_ddim(ref, inp)["sum"],
                         L.oracle_ddim(ref, inp, round_from=0)["sum"], (time.time() - t0) / 2)
        if "b" in cases:
            L.SEED_INPUTS_B = int(opts.get("inputs", L.SEED_INPUTS_B))
            inp, t0 = L.inputs_b(ref), time.time()
            ok &= report(f"b (weights {L.SEED_WEIGHTS_UNET}, inputs {L.SEED_INPUTS_B})", L.oracle_ddpm_tail(ref, inp)["sample"],
                         L.oracle_ddpm_tail(ref, inp, round_from=2)["sample"], (time.time() - t0) / 2)
    if "c" in cases:
        L.SEED_WEIGHTS_SWIN = int(opts.get("weights", L.SEED_WEIGHTS_SWIN))
        L.SEED_INPUTS_C = int(opts.get("inputs", L.SEED_INPUTS_C))
        _, ref = L.swin_nets()
        inp, t0 = L.inputs_c(), time.time()
        ok &= report(f"c (weights {L.SEED_WEIGHTS_SWIN}, inputs {L.SEED_INPUTS_C})", L.oracle_ddim(ref, inp)["sum"],
                     L.oracle_ddim(ref, inp, round_from=0)["sum"], (time.time() - t0) / 2)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
