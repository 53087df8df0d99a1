# Headline bench at (frames in flight, hardware queues) around the default (16, 17)
cd "$GRAFT_REPO_ROOT"
out=${OUT_DIR:-out}/r05ab
mkdir -p $out
for FQ in 16:17 15:16 16:16 14:15 12:13; do
  F=${FQ%:*}; Q=${FQ#*:}
  RTG_BENCH_HW_QUEUES=$Q timeout -k 10 300 python bench.py --full --inflight $F --no-sweep --no-cpu-baseline > $out/inflight_${F}_$Q.log 2>&1 || exit $?
done
