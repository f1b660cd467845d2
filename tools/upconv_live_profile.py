#!/usr/bin/env python3
"""Parent against branch for the live-only upsample + Winograd form (docs/DESIGN_NOTES_upconv_live.md), from two rocprofv3
--kernel-trace CSVs of `bench.py --model vgg --full --steps 10 --warmup 3 --no-check --sustained-s 0 --inflight 1 --tile-policy
energy` (other legs off): one chain, so the launches run in issue order.  The two upsampled F(4x4) layers of a predicted frame are
found by their producers (the stem kernel; the 8 x 8 hand-over through the upsampling); the batched GEMM launched next is the
layer's, the launch after it its consumer.  Averages are over those launches alone (the same kernels also serve other layers).
Usage: upconv_live_profile.py <parent_kernel_trace.csv> <branch_kernel_trace.csv> > profiles/upconv_live_summary.json"""
import csv
import json
import re
import sys
from collections import defaultdict

PRODUCERS = {"upc2 (8x8, 512->512)": "stem_up_input_kernel", "upc3 (16x16, 256->256)": "winograd4_chain_kernel<8, 32, float, false, 512, true"}
PER_ROLLOUT = 10         # predicted frames per rollout: launches of each role


def load(path):
    rows = []
    for r in csv.DictReader(open(path)):
        wg = int(r["Workgroup_Size_X"]) * int(r["Workgroup_Size_Y"]) * int(r["Workgroup_Size_Z"])
        grid = int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"])
        name = re.sub(r"^void dvg::|\(.*$", "", r["Kernel_Name"])
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name, grid // max(wg, 1)))
    rows.sort()
    return rows


def roles(rows):
    """(layer, role) -> {(kernel, workgroups): [durations in us]} of the producer, GEMM and consumer launches."""
    out = defaultdict(lambda: defaultdict(list))
    for i, (_, _, name, _) in enumerate(rows):
        for layer, prod in PRODUCERS.items():
            if not name.startswith(prod):
                continue
            seq = rows[i:i + 3]
            if len(seq) < 3 or not seq[1][2].startswith("conv_igemm2_kernel<3,") or "winograd4_" not in seq[2][2]:
                continue          # (the eager set-up pass packs weights between the launches)
            for role, (s, e, n, g) in zip(("producer", "gemm", "consumer"), seq):
                out[(layer, role)][(n, g)].append((e - s) / 1e3)
    return out


def main():
    out = {"what": __doc__.split("Usage")[0].strip(), "variants": {}, "layers": {}}
    found = {}
    for tag, path in zip(("parent", "branch"), sys.argv[1:3]):
        rows = load(path)
        rollouts = sum(1 for r in rows if r[2].startswith("conv3_wx_kernel<true>")) / 11.0     # 11 first-stage launches per rollout
        gemm = sum(e - s for s, e, n, _ in rows if n.startswith("conv_igemm2_kernel<3,"))
        out["variants"][tag] = {"rollouts": rollouts, "launches": len(rows), "launches_per_rollout": round(len(rows) / rollouts, 2),
                                "kernel_ms_per_rollout": round(sum(e - s for s, e, _, _ in rows) / 1e6 / rollouts, 4),
                                "batched_gemm_ms_per_rollout": round(gemm / 1e6 / rollouts, 4)}
        found[tag] = roles(rows)
    total = {"parent": 0.0, "branch": 0.0}
    for key in sorted(found["parent"]):
        ent = {}
        for tag in ("parent", "branch"):
            (kern, durs), = found[tag][key].items()         # one kernel and grid per role
            avg = sum(durs) / len(durs)
            ent[tag] = {"kernel": kern[0], "workgroups": kern[1], "launches": len(durs), "avg_us": round(avg, 2),
                        "ms_per_rollout": round(avg * PER_ROLLOUT / 1e3, 4)}
            total[tag] += avg * PER_ROLLOUT / 1e3
        ent["branch_over_parent"] = round(ent["branch"]["avg_us"] / ent["parent"]["avg_us"], 3)
        out["layers"][f"{key[0]}: {key[1]}"] = ent
    out["affected_ms_per_rollout"] = {k: round(v, 4) for k, v in total.items()}
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
