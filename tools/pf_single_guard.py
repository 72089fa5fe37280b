"""Guard on the single tick: tools/pf_bench.py on this tree against another build of the library (the parent commit's),
as alternating pairs of runs, each run a process of its own.  Writes one JSON document: per case (model, mode, N) every run's
device tick in ms for both builds, their medians and whether this tree's runs lie inside the other build's own spread.
    bash introtocomputervision_amd/csrc/build.sh                       # in a checkout of the parent commit
    python tools/pf_single_guard.py --parent-lib <parent checkout>/introtocomputervision_amd/libmicv.so \\
        [--pairs 3] [--ticks 200] [--out profiles/pf_group/single_unchanged.json]
The binding loads the other build through MICV_LIB (_capi.py); entry points it lacks are not called by pf_bench.py."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(ticks, lib):
    env = dict(os.environ)
    env.pop("MICV_LIB", None)
    if lib:
        env["MICV_LIB"] = os.path.abspath(lib)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pf_bench.py"), "--ticks", str(ticks), "--ref-ticks", "1"],
                         env=env, capture_output=True, text=True, timeout=300)
    if out.returncode:
        sys.exit(f"pf_bench.py failed ({'parent' if lib else 'this tree'}): rc {out.returncode}\n{out.stderr[-2000:]}")
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pf_group", "single_unchanged.json"))
    a = ap.parse_args()
    cases = {}
    for _ in range(a.pairs):
        for side, lib in (("parent", a.parent_lib), ("this_tree", None)):
            for row in run(a.ticks, lib):
                key = f"{row['model']} {row['mode']} n={row['n']}"
                c = cases.setdefault(key, {"parent": {"tick_dev_ms": [], "seq_host_ms_per_frame": []},
                                           "this_tree": {"tick_dev_ms": [], "seq_host_ms_per_frame": []}})
                c[side]["tick_dev_ms"].append(row["tick_dev_ms"])
                c[side]["seq_host_ms_per_frame"].append(row["seq_host_ms_per_frame"])
    for c in cases.values():
        p, t = c["parent"]["tick_dev_ms"], c["this_tree"]["tick_dev_ms"]
        c["parent_median_ms"], c["this_tree_median_ms"] = statistics.median(p), statistics.median(t)
        c["parent_spread_ms"] = [min(p), max(p)]
        c["this_tree_inside_parent_spread"] = min(p) <= statistics.median(t) <= max(p)
        c["this_tree_over_parent"] = round(statistics.median(t) / statistics.median(p), 4)
    doc = {"tool": "tools/pf_single_guard.py", "what": "micv_pf_tick_dev, ms per tick (tools/pf_bench.py), alternating runs",
           "pairs": a.pairs, "ticks": a.ticks, "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {"parent": v["parent_median_ms"], "this_tree": v["this_tree_median_ms"],
                          "inside": v["this_tree_inside_parent_spread"]} for k, v in cases.items()}))


if __name__ == "__main__":
    main()
