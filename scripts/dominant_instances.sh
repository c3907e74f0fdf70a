cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${1:?usage: bash scripts/dominant_instances.sh OUT_DIR}
mkdir -p $OUT && rm -rf $OUT/prof_dom
CR_BENCH_BF16=0 rocprofv3 --kernel-trace -d $OUT/prof_dom -o p -- python3 bench.py --full --no-cpu-baseline > $OUT/dom_bench.json 2> $OUT/dom_bench.err
DB=$(ls $OUT/prof_dom/*.db $OUT/prof_dom/*/*.db 2>/dev/null | head -1)
python scripts/dominant_instances.py $DB $OUT/dom_bench.json $OUT/dominant.json
rm -rf $OUT/prof_dom
