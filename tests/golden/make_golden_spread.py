#!/usr/bin/env python3
"""Spread-score goldens from the REAL reference model (build container only; needs /root/reference).

For every case of tests/spread_ref.py (tiny, 2M, 6M, 85M and the two extra shapes) this writes tests/golden/gptspread_<case>.npz with
    logits_f32   float32 [136, 67]  mapf_gpt/model.py GPT.forward in fp32 on the first 136 rows of gptbig_2M_s1 tokens (85M: 129 rows)
    logits_f64   float64 [136, 67]  the same module after .double()                      (the accuracy yardstick)
    logits_bf16  float32 [136, 67]  the same module under torch.autocast(bfloat16)
    factor, seed                    the q/k factor of spread_ref.FACTORS and the seed of the synthetic weights
    spread, fb_lo, fb_hi  float64 [n_layer]   spread_ref.regime on the oracle port over the case's first REGIME_ROWS rows
    regime_rows
2M and 6M also get gptspread_<case>_nopos.npz: the same for the permutation test's wpe = 0 checkpoint (factor of spread_ref.FACTORS_NOPOS,
regime figures over PERM_REGIME_ROWS rows).
No tokens and no weights are stored: both are regenerated from seeds.  The generated files are data only; nothing at test time reads
/root/reference.
Run:  python tests/golden/make_golden_spread.py [case ...]
"""
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")

from tests import spread_ref  # noqa: E402


def import_reference_model():
    sys.path.insert(0, "/root/reference")
    lg = types.ModuleType("loguru")
    lg.logger = type("L", (), {"__getattr__": lambda s, k: (lambda *a, **kw: None)})()
    sys.modules["loguru"] = lg
    from mapf_gpt.model import GPT, GPTConfig
    return GPT, GPTConfig


def regime_arrays(sd, args, tok):
    r = np.array(spread_ref.regime(sd, args, tok), dtype=np.float64)
    return dict(spread=r[:, 0], fb_lo=r[:, 1], fb_hi=r[:, 2], regime_rows=np.array(len(tok)))


def main():
    import torch
    GPT, GPTConfig = import_reference_model()
    torch.set_num_threads(8)
    seed = 0
    for case in (sys.argv[1:] or spread_ref.CASES):
        for nopos in ((False, True) if case in ("2M", "6M") else (False,)):
            args = spread_ref.case_args(case)
            rows = spread_ref.tokens(spread_ref.n_fixture_rows(case))
            idx = torch.from_numpy(rows.astype(np.int64))
            sd = spread_ref.spread_state_dict(args, seed=seed, nopos=nopos)
            net = GPT(GPTConfig(**args)).eval()
            net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
            t0 = time.time()
            outs = {}
            with torch.no_grad():
                outs["logits_f32"] = torch.cat([net(idx[i:i + 32])[0][:, 0, :] for i in range(0, len(idx), 32)]).numpy().astype(np.float32)
                with torch.autocast(device_type="cpu", dtype=torch.bfloat16):
                    outs["logits_bf16"] = torch.cat([net(idx[i:i + 32])[0][:, 0, :].float() for i in range(0, len(idx), 32)]).numpy().astype(np.float32)
                net64 = net.double()
                outs["logits_f64"] = torch.cat([net64(idx[i:i + 32])[0][:, 0, :] for i in range(0, len(idx), 32)]).numpy().astype(np.float64)
            factor = (spread_ref.FACTORS_NOPOS if nopos else spread_ref.FACTORS)[(args["n_layer"], args["n_head"], args["n_embd"])]
            reg = regime_arrays(sd, args, rows[:spread_ref.PERM_REGIME_ROWS if nopos else spread_ref.REGIME_ROWS[case]])
            tag = f"gptspread_{case}" + ("_nopos" if nopos else "")
            np.savez_compressed(os.path.join(OUT, tag + ".npz"), factor=np.array(factor), seed=np.array(seed), **reg, **outs)
            e32 = np.abs(outs["logits_f32"] - outs["logits_f64"]).max()
            e16 = np.abs(outs["logits_bf16"] - outs["logits_f64"]).max()
            print(f"{tag}: factor {factor}  max|logit| {np.abs(outs['logits_f64']).max():.3f}  fp32-fp64 {e32:.2e}  autocast-fp64 {e16:.2e}  "
                  f"spread {reg['spread'].min():.1f}..{reg['spread'].max():.1f}  fb_lo {reg['fb_lo'].min():.3f}..{reg['fb_lo'].max():.3f}  "
                  f"fb_hi {reg['fb_hi'].min():.3f}..{reg['fb_hi'].max():.3f}  ({time.time() - t0:.0f} s)", flush=True)

if __name__ == "__main__":
    main()
