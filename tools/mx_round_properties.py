"""The two properties MX round tuning relies on, counted on the torch restatement -- no GPU needed.

For each of the 6 formats x 4 scale rules, on `--blocks` random blocks of 32 (Gaussian values, one block scale each, uniform over
2^-100 .. 2^100; generator seed `--seed`) and uniform random selections:
  (a)  elements where `where(rounding > .5, hi, lo)` has other bits than `mx_fake_quant(w)` although `rounding != .5`
  (b)  blocks that `mx_fake_quant(out, rule)` changes, and blocks whose code it changes
The counts of (b) under MXFP8_E4M3 / EVEN and of the changed codes depend on the draw; the zeros do not.

    python tools/mx_round_properties.py [--blocks 61440] [--seed 2026]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from ppq_amd import MXFormat, MXScaleRule, mx_fake_quant, mx_round_forward, mx_round_split
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=61440)
    ap.add_argument('--seed', type=int, default=2026)
    args = ap.parse_args()
    g = torch.Generator().manual_seed(args.seed)
    x = torch.randn(args.blocks, 32, generator=g) * torch.exp2(torch.randint(-100, 101, (args.blocks, 1), generator=g).float())
    selection = torch.rand(args.blocks, 32, generator=g)
    print(f'# tools/mx_round_properties.py --blocks {args.blocks} --seed {args.seed}')
    for fmt in MXFormat:
        for rule in MXScaleRule:
            floored, rounding, codes = mx_round_split(x, fmt, -1, rule, use_kernels=False)
            nearest = mx_round_forward(floored, rounding, codes, fmt, -1, use_kernels=False)
            fq = mx_fake_quant(x, fmt, -1, use_kernels=False, scale_rule=rule)
            a = int(((nearest.view(torch.int32) != fq.view(torch.int32)) & (rounding != .5)).sum())
            out = mx_round_forward(floored, selection, codes, fmt, -1, use_kernels=False)
            again_codes = torch.zeros_like(codes)
            again = mx_fake_quant(out, fmt, -1, scale_codes=again_codes, use_kernels=False, scale_rule=rule)
            b = int((again.view(torch.int32) != out.view(torch.int32)).any(dim=-1).sum())
            print(f'{fmt.name:11s} {rule.name:5s} (a) mismatches {a}   (b) blocks changed {b}   codes changed {int((again_codes != codes).sum())}   '
                  f'exact ties {int((rounding == .5).sum())}')


if __name__ == '__main__':
    main()
