# Round-4 measurement set (run on the GPU box through gpurun): bench lines, rocprofv3 kernel stats, HBM traffic (two PMC passes
# each) and SQ counters of the one-image step and of ONE 8-image batch on one stream; kernel stats of the crop (close-up) regime;
# kernel stats + matrix-core counters of the geometry decoder.  Summaries land in gpurun_out/r04/ -- copy them to profiles/r04_*.
R=${GRAFT_REPO_ROOT:-/root/repo}
O=$R/gpurun_out/r04
mkdir -p $O
export TMPDIR=/tmp
cd $R
timeout 1200 python bench.py --full > $O/bench_b1.json 2> $O/bench_b1.err
timeout 600 python bench.py --full --steps 20 --warmup 5 > $O/bench_driver_invocation.json 2>/dev/null
timeout 300 python bench.py --full --no-cpu-baseline --no-extras --steps 200 --warmup 50 --images-per-gpu 8 > $O/bench_b8.json 2>/dev/null
timeout 300 python bench.py --full --no-cpu-baseline --no-extras --steps 200 --warmup 50 --images-per-gpu 32 > $O/bench_b32.json 2>/dev/null
cd /tmp
B1="python $R/bench.py --full --steps 100 --warmup 10 --no-cpu-baseline --no-extras"
NG="python $R/bench.py --full --steps 20 --warmup 2 --repeats 1 --no-cpu-baseline --no-extras --no-graph"
timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/kt_b1 -- $B1 > /dev/null 2>&1
timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/kt_b8 -- $B1 --images-per-gpu 8 --streams 1 > /dev/null 2>&1
timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/kt_c1 -- python $R/scripts/run_steps.py --crop hoi --steps 300 > /dev/null 2>&1
timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/kt_c8 -- python $R/scripts/run_steps.py --crop hoi --images 8 --streams 1 --steps 100 > /dev/null 2>&1
timeout -k 5 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/kt_geo -- python $R/scripts/geo_bench.py --fb > /dev/null 2>&1
for t in b1 b8; do
  X=""; [ $t = b8 ] && X="--images-per-gpu 8 --streams 1"
  timeout 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/d_fetch_$t -- $NG $X > /dev/null 2>&1
  timeout 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/d_write_$t -- $NG $X > /dev/null 2>&1
  timeout 300 rocprofv3 --pmc TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_32B_sum TCC_EA0_RDREQ_64B_sum TCC_EA0_RDREQ_128B_sum --output-format csv -d $O/d_eard_$t -- $NG $X > /dev/null 2>&1
  timeout 300 rocprofv3 --pmc TCC_EA0_WRREQ_sum TCC_EA0_WRREQ_64B_sum TCC_EA0_ATOMIC_sum --output-format csv -d $O/d_eawr_$t -- $NG $X > /dev/null 2>&1
  timeout 300 rocprofv3 --pmc SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY --output-format csv -d $O/d_sqa_$t -- $NG $X > /dev/null 2>&1
  timeout 300 rocprofv3 --pmc GRBM_GUI_ACTIVE SQ_INSTS_VALU SQ_INSTS_SALU SQ_ACTIVE_INST_VALU SQ_INSTS_LDS --output-format csv -d $O/d_sqb_$t -- $NG $X > /dev/null 2>&1
done
# the geometry decoder: matrix-core busy cycles, VALU / LDS instruction mix, waits
GB="python $R/scripts/geo_bench.py --fb"   # HIP decoder only: three forward + backward passes, three forwards
timeout 300 rocprofv3 --pmc SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU --output-format csv -d $O/d_geo1 -- $GB > /dev/null 2>&1
timeout 300 rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_LDS SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_INSTS_MFMA SQ_ACTIVE_INST_LDS GRBM_GUI_ACTIVE --output-format csv -d $O/d_geo2 -- $GB > /dev/null 2>&1
timeout 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/d_geo3 -- $GB > /dev/null 2>&1
timeout 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/d_geo4 -- $GB > /dev/null 2>&1
cd $R
for t in b1 b8 c1 c8 geo; do find $O/kt_$t -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $O/kernel_stats_$t.csv; done
for t in b1 b8; do
  python scripts/summarize_pmc.py $(find $O/d_fetch_$t $O/d_write_$t -name "*counter_collection.csv") > $O/pmc_fetch_write_$t.csv
  python scripts/summarize_pmc.py $(find $O/d_sqa_$t $O/d_sqb_$t -name "*counter_collection.csv") > $O/sq_counters_$t.csv
  python scripts/summarize_pmc.py $(find $O/d_eard_$t $O/d_eawr_$t -name "*counter_collection.csv") > $O/ea_requests_$t.csv
done
python scripts/summarize_pmc.py $(find $O/d_geo1 $O/d_geo2 $O/d_geo3 $O/d_geo4 -name "*counter_collection.csv") > $O/geo_counters.csv
rm -rf $O/kt_* $O/d_*
ls -la $O; head -9 $O/kernel_stats_b1.csv | cut -c1-110; head -9 $O/kernel_stats_c1.csv | cut -c1-110; grep geo $O/kernel_stats_geo.csv | cut -c1-130
