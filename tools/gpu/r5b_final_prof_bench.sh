set -e
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
bash tools/gpu/final_prof.sh
O=${OUT_DIR:-bench_out}/r5final
mkdir -p $O
python bench.py --full > $O/bench.json 2> $O/bench.err || { tail -30 $O/bench.err; exit 1; }
python - <<PY
import json
d=json.loads(open("$O/bench.json").read().strip().splitlines()[-1])
r=d["roofline"]
print("value", d["value"], "frac", r["frac"], "lba_alone", r["lba_alone"].get("frac_of_fp64_peak"), [x.get("frac_of_fp64_peak") for x in r["lba_alone_by_batch"]], "stereo", d["stereo"]["frames_per_s"], "bases32", d["bases32"]["frames_per_s"], "frontend", d["frontend"]["frames_per_s"], "failed", d["extras_failed"], "rss", d["host_max_rss_gb"])
PY
