#!/usr/bin/env python3
"""Same-box A/B of several builds of the library on the headline run WITH its roofline leg: images/s and the in-situ launch time of the
dominant kernel kind (bench.py's ``roofline.avg_launch_ms``: one event pair per forward inside the steady-state forward, the chip at the
clock the whole instruction mix gives it), builds alternated round by round.  Every bench line is kept in <out>/<build>_r<round>.json.
    python scripts/ab_insitu.py build_ab/parent.so build_ab/new.so [--rounds 3] [--out build_ab/ab_insitu] [--box] [bench.py args...]"""
import json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
rounds, out, box = 3, os.path.join(ROOT, "build_ab", "ab_insitu"), False
if "--rounds" in args:
    i = args.index("--rounds"); rounds = int(args[i + 1]); del args[i:i + 2]
if "--out" in args:
    i = args.index("--out"); out = args[i + 1]; del args[i:i + 2]
if "--box" in args:
    args.remove("--box"); box = True
libs = [a for a in args if a.endswith(".so")]
rest = [a for a in args if not a.endswith(".so")]
os.makedirs(out, exist_ok=True)
res = {l: [] for l in libs}
for r in range(rounds):
    for l in libs:
        name = os.path.basename(l)[:-3]
        env = dict(os.environ, PD_ALLOW_ABI_MISMATCH="1", PD_LIB=os.path.abspath(l))
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-sweep",
               "--no-side-workloads"] + ([] if box else ["--no-box"]) + rest
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=400)
        if p.returncode != 0:
            print(f"!! {name}: exit {p.returncode}: {p.stderr[-600:]}", flush=True)
            if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
                sys.exit(1)          # a crash or a time limit: nothing more is started on this GPU
            continue
        line = p.stdout.strip().splitlines()[-1]
        open(os.path.join(out, f"{name}_r{r}.json"), "w").write(line + "\n")
        d = json.loads(line)
        rf = d.get("roofline") or {}
        res[l].append((d["value"], d["ms_per_step"], rf.get("kernel"), rf.get("avg_launch_ms"), rf.get("avg_launch_ms_in_situ_by_launch"), d.get("box")))
        print(f"round {r} {name:14s} {d['value']:8.3f} img/s  {d['ms_per_step']:9.2f} ms/step  {rf.get('kernel')} in situ {rf.get('avg_launch_ms')} ms "
              f"{rf.get('avg_launch_ms_in_situ_by_launch')}", flush=True)
for l in libs:
    if res[l]:
        v = [x[0] for x in res[l]]
        t = [x[3] for x in res[l] if x[3] is not None]
        print(f"{os.path.basename(l)[:-3]:14s} img/s median {statistics.median(v):8.3f} [{min(v):.3f} .. {max(v):.3f}]   "
              + (f"{res[l][0][2]} in situ median {statistics.median(t):.4f} ms [{min(t):.4f} .. {max(t):.4f}]" if t else ""))
