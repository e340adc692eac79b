# bench.py configs 3 / 4 / 5 with every leg (--full; config 2 is the default run) -> $OUT/bench_c*.log
set -u
OUT=${OUT:-out}
mkdir -p $OUT
for c in 3 4 5; do
  timeout -k 10 600 python bench.py --full --config $c > $OUT/bench_c$c.log 2>&1 || { echo "config $c failed"; exit 1; }
done
