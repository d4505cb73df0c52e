#!/bin/bash
# Round-3 profile set (run on the GPU box through gpurun; outputs under gpurun_out/$TAG, summaries are copied to profiles/
# by tools/prof/r03_collect.py).  Usage: tools/prof/r03_profile.sh <tag>
TAG=${1:-r03a}
ROOTD=$PWD
cd /tmp && export TMPDIR=/tmp; cd $ROOTD
OUT=gpurun_out/$TAG; mkdir -p $OUT; : > $OUT/bench.err
# 2. kernel trace + stats of the same command (10 slots x 4 steps per launch in flight) and of the single-stream run (clean kernel times)
rocprofv3 --kernel-trace --stats -d $OUT/kt20 -o kt -- python bench.py --full --steps 256 --no-cpu-baseline --no-parity --steady-steps 0 > $OUT/bench_under_rocprof.json 2>> $OUT/bench.err
rocprofv3 --kernel-trace --stats -d $OUT/kt1 -o kt -- python bench.py --full --steps 64 --warmup 4 --streams 1 --no-cpu-baseline --no-parity --steady-steps 0 > $OUT/bench_streams1.json 2>> $OUT/bench.err
# 3. HBM traffic (separate PMC passes, single stream so that launches do not overlap)
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/pmc_fetch -o f -- python bench.py --full --steps 8 --warmup 2 --streams 1 --no-cpu-baseline --no-parity --steady-steps 0 > /dev/null 2>> $OUT/bench.err
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/pmc_write -o w -- python bench.py --full --steps 8 --warmup 2 --streams 1 --no-cpu-baseline --no-parity --steady-steps 0 > /dev/null 2>> $OUT/bench.err
# 4. what bounds the solve: issue / LDS counters (two passes of 8 SQ counters); --gang 1: 256-scene launches = ONE wave per CU
rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS --kernel-trace --output-format csv -d $OUT/pmc_sq_a -o a -- python bench.py --full --steps 8 --warmup 2 --streams 1 --gang 1 --no-cpu-baseline --no-parity --steady-steps 0 > /dev/null 2>> $OUT/bench.err
rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_SALU SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_LDS_ADDR_CONFLICT SQ_WAVES GRBM_GUI_ACTIVE --kernel-trace --output-format csv -d $OUT/pmc_sq_b -o b -- python bench.py --full --steps 8 --warmup 2 --streams 1 --gang 1 --no-cpu-baseline --no-parity --steady-steps 0 > /dev/null 2>> $OUT/bench.err
find $OUT -name "*.csv" -o -name "*.db" | head -40
tail -3 $OUT/bench.err
# 1. the summaries bench.py quotes (profiles/r03_*: rocprofv3's durations and PMC traffic of these very commands), then the bench
#    line itself (default: 2048 steps) and the 20-step line the driver asks for
python tools/experiments/ms_parts.py > $OUT/ms_parts.txt 2>> $OUT/bench.err
python tools/prof/r03_collect.py $TAG --profiles-only
python bench.py --full > $OUT/bench.json 2>> $OUT/bench.err
python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-parity > $OUT/bench_20steps.json 2>> $OUT/bench.err
# 5. the collective path on one GPU: bench.py under torch.distributed.run with one rank (one ncclAllGather per sweep, amk_shard_gather)
python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29517 bench.py --full --gpus 1 --no-cpu-baseline --no-parity > $OUT/bench_torchrun_1rank.json 2>> $OUT/bench.err
# 6. other BASELINE sizes and launch shapes (not the headline)
python bench.py --full --points 200000 --T 1.0 --steps 64 --warmup 4 --streams 8 --no-cpu-baseline --no-parity --steady-steps 0 > $OUT/bench_c5size.json 2>> $OUT/bench.err
python bench.py --full --points 5000 --T 0.33 --K 3 --steps 512 --no-cpu-baseline --no-parity --steady-steps 0 > $OUT/bench_c1size.json 2>> $OUT/bench.err
python bench.py --full --steps 64 --warmup 4 --scenes 1 --streams 1 --gang 1 --no-cpu-baseline --no-parity --steady-steps 0 > $OUT/bench_single_robot.json 2>> $OUT/bench.err
python bench.py --full --steps 32 --warmup 4 --scenes 2048 --streams 1 --gang 1 --no-cpu-baseline --no-parity --steady-steps 0 > $OUT/bench_s2048_streams1.json 2>> $OUT/bench.err
python bench.py --full --ipm-max-iter 40 --no-cpu-baseline --no-parity > $OUT/bench_cap40.json 2>> $OUT/bench.err
python bench.py --full --streams 20 --gang 1 --no-cpu-baseline --no-parity > $OUT/bench_20x1.json 2>> $OUT/bench.err
python bench.py --full --streams 20 --gang 1 --steps 20 --warmup 5 --no-cpu-baseline --no-parity > $OUT/bench_20x1_20steps.json 2>> $OUT/bench.err
python tools/experiments/burst_timeline.py 10 4 20 > $OUT/burst_timeline_10x4.txt 2>> $OUT/bench.err
python tools/experiments/burst_timeline.py 20 1 20 > $OUT/burst_timeline_20x1.txt 2>> $OUT/bench.err
python tools/experiments/exact_mode_cost.py > $OUT/exact_mode_cost.txt 2>> $OUT/bench.err
for c in a b; do for qd in 1 8; do QD=$qd python tools/experiments/rccl_presence.py $c 2>/dev/null | grep "^case . *: [0-9]" | sed "s/^/QD=$qd /" >> $OUT/rccl_presence.txt; done; done
cat $OUT/exact_mode_cost.txt $OUT/rccl_presence.txt
cat $OUT/ms_parts.txt
ls $OUT
