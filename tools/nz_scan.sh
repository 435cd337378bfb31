#!/bin/bash
# one box: cost per site against the number of planes (256 x 256 x nz)
run() { python bench.py --full --shape $1 --steps 60 --warmup 10 --no-cpu-baseline 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.readline()); print('%-14s %-22s %8.1f MLUPS %8.4f ms' % ('$1', '$2', d['value'], d['ms_per_step']))"; }
for nz in 128 192 224 240 248 256 264 272 288 320 384; do run 256,256,$nz "-"; done
