O=${1:-$(mktemp -d)}     # output directory (default: a fresh temporary one)
mkdir -p $O
export COGS_BENCH_REHEARSAL=1
S=$(date +%s)
timeout -k 10 600 python bench.py --full --gpus 2 --steps 3 --warmup 1 > $O/bench2.json 2> $O/bench2.err
echo "rc $? wall $(( $(date +%s) - S )) s"
python - "$O/bench2.json" <<'PY'
import json, sys
d=json.loads([l for l in open(sys.argv[1]) if l.startswith("{")][0])
print(d["value"], d["n_gpus"], d["ranks_seen"], d["ms_per_step"]); print(json.dumps(d["allgather"], indent=1)); print(d.get("wall_s")); print(d["cfg3"]["value"], d["weak"]["value"])
PY
tail -3 $O/bench2.err
