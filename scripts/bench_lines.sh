#!/bin/bash
# Every workload's bench line with its CPU baseline (on an MI355X, from the repo root; OUT = a directory for the results):
#   OUT=<dir> bash scripts/bench_lines.sh > <dir>/bench_lines.jsonl      -> profiles/<round>_bench_lines.jsonl
# and the one-GPU --full command (headline + `secondary`) into <dir>/bench_default_line.json
: "${OUT:?set OUT to the directory the results go to}"
python bench.py --full --steps 200 --warmup 20 --no-secondary --no-live-counters 2>/dev/null | tail -1
for w in xy ddp srb walk multi xywalk ism z ddpzmp; do python bench.py --workload $w --no-live-counters 2>/dev/null | tail -1; done
python bench.py --full 2>/dev/null | tail -1 > "$OUT"/bench_default_line.json
