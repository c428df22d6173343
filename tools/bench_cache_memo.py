"""Host cost of a WARM HIT of the weight-derived operand caches (pna_amd/_cache.py): what every call of a fast path
pays in the interpreter before its first launch.

    python tools/bench_cache_memo.py [--device cpu|cuda] [--number 2000] [--repeat 5] [--out FILE]

Times the builders at the shapes of tests/test_cache_coherence_host.py (4 towers of 20 features) with timeit: `repeat` repeats of `number`
calls each, gc disabled by timeit; per builder the median and the spread (max - min) of the repeats, in microseconds per call.  The
interpreter work does not depend on where the tensors live except for the device part of the key, so --device cpu serves for the
pure-torch builders; pack_posttrans_weight builds with a kernel and is timed on --device cuda only.  The script calls the builders by
the names they have had since the caches exist, so the same file run from a checkout of an earlier commit gives that commit's numbers
(profiles/cache_memo_host.json holds both)."""
import argparse
import json
import os
import statistics
import sys
import timeit

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

AGGS, SCALERS = "mean max min std", "identity amplification attenuation"


def builders(dev):
    from pna_amd import functional as PF, ops
    from pna_amd.dgl import pna_layer as PL
    torch.manual_seed(0)
    layer = PL.PNALayer(20, 20, AGGS, SCALERS, {"log": torch.tensor(1.3)}, 0.0, True, True, towers=4, divide_input=False, residual=True).eval().to(dev)
    layer16 = PL.PNALayer(20, 20, AGGS, SCALERS, {"log": torch.tensor(1.3)}, 0.0, True, True, towers=4, divide_input=False,
                          residual=True).eval().to(dev).to(torch.bfloat16)
    towers, mix = list(layer.towers), layer.mixing_network
    towers16, mix16 = list(layer16.towers), layer16.mixing_network
    bn = towers[0].batchnorm_h

    def collapsed_and_pass():
        PF._tower_collapsed_weights(layer, towers, mix, False)
        PF._tower_pass_weights(layer, towers, mix)
    out = {
        "_fold_batchnorm": lambda: PF._fold_batchnorm(bn),
        "_projection_cache": lambda: PL._projection_cache(towers, 20),
        "_tower_collapsed_weights + _tower_pass_weights": collapsed_and_pass,
        "_small_images_bf16": lambda: PF._small_images_bf16(towers16, mix16, False),
        "_tower_images_bf16": lambda: PF._tower_images_bf16(towers16, False),
    }
    if dev.type == "cuda":
        w = towers[0].posttrans.fully_connected[0].linear.weight                 # (20, 20 + 3 * 80): [h | three scaler blocks]
        out["pack_posttrans_weight"] = lambda: ops.pack_posttrans_weight(w, 80, 3, 20)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--number", type=int, default=2000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {}
    with torch.no_grad():
        for name, fn in builders(torch.device(args.device)).items():
            fn(), fn()                                                          # build, then one warm hit
            us = [t / args.number * 1e6 for t in timeit.repeat(fn, number=args.number, repeat=args.repeat)]
            res[name] = {"median_us": round(statistics.median(us), 3), "spread_us": round(max(us) - min(us), 3), "repeats_us": [round(u, 3) for u in us]}
            print(f"{name:50s} {res[name]['median_us']:8.3f} us  (spread {res[name]['spread_us']:.3f})", flush=True)
    out = {"device": args.device, "number": args.number, "repeat": args.repeat, "warm_hit": res}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
