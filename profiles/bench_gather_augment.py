"""Batch assembly at the flagship shape (batch 32, 3+1 channels, 320 x 427, a dataset arena of 512 rows, 1.12 GB):
what gsd_gather_augment costs against the two gsd_gather_affine launches it replaces, against a plain device-to-device copy
of the same bytes, and against the fp32 train step it feeds.

    python profiles/bench_gather_augment.py [--launches 400] [--out FILE.json] [--no-step]
    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/bench_gather_augment.py --launches 100 --no-step --no-events

Every launch takes its rows from another batch of a shuffled pass over the arena (16 batches of 32 rows: the working set is
the whole 1.12 GB, nothing is served from a cache that a training pass would not have).  Times are medians of per-launch device
event pairs; bytes are the algorithm's own (rows read once, batch written once).  The acceptance line: the fully augmented
launch takes no more than 1 % of the fp32 batch-32 train step measured in the same process."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

B, CI, CD, H, W, M = 32, 3, 1, 320, 427, 512
DIMS = [64, 128, 256, 512, 1024]


def timed(fn, batches, launches, warmup, events=True):
    """Median / min / mean microseconds of fn(batch index) over `launches` launches, one device event pair per launch."""
    for k in range(warmup):
        fn(k % batches)
    torch.cuda.synchronize()
    if not events:
        for k in range(launches):
            fn(k % batches)
        torch.cuda.synchronize()
        return None
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for k, (a, b) in enumerate(pairs):
        a.record()
        fn(k % batches)
        b.record()
    torch.cuda.synchronize()
    us = [1e3 * a.elapsed_time(b) for a, b in pairs]
    return {"median_us": statistics.median(us), "min_us": min(us), "mean_us": statistics.fmean(us), "launches": launches}


def step_ms(steps=10, warmup=3):
    from gelslim_depth_amd import synth
    from gelslim_depth_amd.models.unet import UNet
    from gelslim_depth_amd.train import TrainStep
    m = UNet(n_channels=3, n_classes=1, layer_dimensions=DIMS, precision="fp32")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state(3, 1, DIMS, 0, "conditioned").items()}, strict=True)
    step = TrainStep(m.to("cuda").train(), lr=1e-3, weight_decay=1e-6, ema_decay=0.995, loss="mse")
    x, t = torch.rand((B, 3, H, W), device="cuda"), -0.9 * torch.rand((B, 1, H, W), device="cuda")
    for _ in range(warmup):
        step(x, t)
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step(x, t)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=32)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-step", action="store_true", help="skip the train step (profiler runs)")
    ap.add_argument("--no-events", action="store_true", help="launch only, time nothing (profiler runs)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_gather_augment: needs the GPU (a CPU run measures nothing)")
    from gelslim_depth_amd.dataset import Augment, gather_affine, gather_augment
    dev = "cuda"
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    img = 255.0 * torch.rand((M, CI, H, W), device=dev, generator=g)
    dep = -2.0 * torch.rand((M, CD, H, W), device=dev, generator=g)
    flat = torch.cat([img.view(-1), dep.view(-1)])          # the copy's source: the same 1.12 GB
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(2)).to(dev)
    idx = [perm[k * B:(k + 1) * B].contiguous() for k in range(M // B)]
    Ai = torch.tensor([1 / 41.3, 1 / 38.9, 1 / 45.2], device=dev)
    Bi = torch.tensor([-121.7 / 41.3, -130.2 / 38.9, -117.5 / 45.2], device=dev)
    Ad, Bd = torch.tensor([-0.466], device=dev), torch.tensor([-0.009], device=dev)
    out = (torch.empty((B, CI, H, W), device=dev), torch.empty((B, CD, H, W), device=dev))
    n_out = out[0].numel() + out[1].numel()
    dst = torch.empty((n_out,), device=dev)
    augs = {"augment identity": Augment(),
            "augment geometry": Augment(seed=1, hflip=0.5, vflip=0.5, max_shift=(8, 8)),
            "augment gain+offset": Augment(seed=1, hflip=0.5, vflip=0.5, max_shift=(8, 8), gain=0.2, offset=10.0, pivot=127.5),
            "augment full": Augment(seed=1, hflip=0.5, vflip=0.5, max_shift=(8, 8), gain=0.2, offset=10.0, noise_std=3.0,
                                    pivot=127.5)}

    def two_plain(k):
        gather_affine(img, idx[k], Ai, Bi)
        gather_affine(dep, idx[k], Ad, Bd)
    cases = {"two gather_affine": two_plain,
             "copy d2d": lambda k: dst.copy_(flat[k * n_out:(k + 1) * n_out])}
    for name, aug in augs.items():
        st = aug.struct(3)
        cases[name] = lambda k, st=st: gather_augment(img, dep, idx[k], Ai, Bi, Ad, Bd, st, out=out)
    nbytes = 2 * 4 * n_out
    rows = {}
    for rep in range(2):        # two interleaved rounds: the second is reported, the first shows the spread
        for name, fn in cases.items():
            r = timed(fn, len(idx), args.launches, args.warmup, events=not args.no_events)
            if r is not None:
                r["first_round_median_us"] = rows.get(name, r)["median_us"]
                rows[name] = r
    if args.no_events:
        print("launched", 2 * args.launches, "of each case, untimed")
        return
    copy_rate = nbytes / rows["copy d2d"]["median_us"] / 1e6
    for name, r in rows.items():
        r["TB_per_s"] = nbytes / r["median_us"] / 1e6
        r["share_of_copy_rate"] = r["TB_per_s"] / copy_rate
        r["ratio_to_two_gather_affine"] = r["median_us"] / rows["two gather_affine"]["median_us"]
    res = {"shape": {"B": B, "Ci": CI, "Cd": CD, "H": H, "W": W, "arena_rows": M}, "bytes_per_launch": nbytes,
           "device": torch.cuda.get_device_name(0), "cases": rows}
    if not args.no_step:
        res["fp32_step_ms"] = step_ms()
        res["limit_us"] = 10.0 * res["fp32_step_ms"]            # 1 % of the step
        res["full_share_of_step"] = rows["augment full"]["median_us"] / (1e3 * res["fp32_step_ms"])
        res["accepted"] = bool(rows["augment full"]["median_us"] <= res["limit_us"])
    print(f"{'case':24s} {'median us':>10s} {'min us':>8s} {'1st round':>10s} {'TB/s':>6s} {'of copy':>8s} {'vs 2 plain':>10s}")
    for name, r in rows.items():
        print(f"{name:24s} {r['median_us']:10.1f} {r['min_us']:8.1f} {r['first_round_median_us']:10.1f} {r['TB_per_s']:6.2f} "
              f"{r['share_of_copy_rate']:8.2f} {r['ratio_to_two_gather_affine']:10.2f}")
    if "fp32_step_ms" in res:
        print(f"fp32 batch-32 train step {res['fp32_step_ms']:.2f} ms; augment full = {100 * res['full_share_of_step']:.3f} % of it "
              f"(limit 1 %): {'ok' if res['accepted'] else 'TOO SLOW'}")
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    if "accepted" in res and not res["accepted"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
