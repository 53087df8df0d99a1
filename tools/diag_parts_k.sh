cd "$GRAFT_REPO_ROOT"
out=${OUT_DIR:-out}/r05t
mkdir -p $out
for K in 1000 10000 100352; do
  timeout -k 10 300 python bench.py --full --K $K --steps 40 --no-sweep --no-cpu-baseline > $out/parts_K$K.log 2>&1 || exit $?
done
