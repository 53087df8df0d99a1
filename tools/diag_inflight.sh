# Headline bench (parts prediction included) at 16 / 24 / 31 frames in flight, one hardware queue
# per replica stream + 1 (RTG_BENCH_HW_QUEUES; the box refuses more than 32)
cd "$GRAFT_REPO_ROOT"
out=${OUT_DIR:-out}/r05aa
mkdir -p $out
for F in 16 24 31; do
  RTG_BENCH_HW_QUEUES=$((F + 1)) timeout -k 10 300 python bench.py --full --inflight $F --no-sweep --no-cpu-baseline > $out/inflight_$F.log 2>&1 || exit $?
done
