# A/B of one environment variable's values on ONE box: bash scripts/ab_envval.sh VAR v1 v2 ...   (bench.py, two rounds)
cd $GRAFT_REPO_ROOT
VAR=$1; shift
T=$(mktemp -d)
for rep in 1 2; do
for v in "$@"; do
  export $VAR=$v
  timeout -k 10 200 python bench.py --full --steps 20 --warmup 3 --no-cpu-baseline > "$T/b.json" 2> "$T/b.log"
  echo "$VAR=$v: $(grep -o 'timed region done: [0-9.]* ms/step' "$T/b.log") $(grep -o 'stash mode: [0-9.]* ms/step' "$T/b.log")"
done; done
