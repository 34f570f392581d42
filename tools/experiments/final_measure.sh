#!/bin/bash
# round-end measurement set (run on the GPU box through gpurun; every tool call is bounded by its own timeout)
export TMPDIR=/tmp
o=${1:?usage: final_measure.sh OUTDIR}
mkdir -p $o
timeout 250 python bench.py --full > $o/bench_v8.json 2> $o/bench_v8.err
timeout -s KILL 200 rocprofv3 --kernel-trace --stats --output-format csv -d $o/prof -o kt -- python bench.py --full --steps 5 --warmup 1 --no-cpu-baseline > $o/prof.log 2>&1
timeout -s KILL 240 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $o/pmc_fetch -o f -- python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $o/pmc_fetch.log 2>&1
timeout -s KILL 240 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $o/pmc_write -o w -- python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $o/pmc_write.log 2>&1
timeout 400 python bench.py --full --config tdt-600m --bf16 --steps 8 --warmup 2 > $o/bench_600m_bf16.json 2> $o/bench_600m_bf16.err
ls -la $o $o/prof | head -40
