#!/bin/sh
# Resource table of the fp32 evaluation-row kernels that share csrc/f32_tile.h, for one source tree (no GPU needed):
#   scripts/f32_rows_resources.sh [csrc directory]
# One line a kernel from -Rpass-analysis=kernel-resource-usage (VGPRs, scratch, occupancy, LDS) plus the MFMA instructions of the
# file's gfx950 assembly.  Run it over two trees and diff the outputs.
set -e
CSRC=${1:-$(dirname "$0")/../difashion_amd/csrc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result -mllvm -amdgpu-mfma-vgpr-form=1 --cuda-device-only"
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
for f in clip eval_scores lpips; do
  extra=""
  [ "$f" = lpips ] && extra="-ffp-contract=off"
  hipcc $FLAGS $extra -Rpass-analysis=kernel-resource-usage -S "$CSRC/$f.hip" -o "$TMP/$f.s" 2> "$TMP/$f.txt"
  awk -v file="$f.hip" '
    /Function Name:/ { name = $(NF-1) }
    / VGPRs:/ { v = $(NF-1) }
    /ScratchSize/ { s = $(NF-1) }
    /Occupancy/ { o = $(NF-1) }
    /LDS Size/ { printf "%-12s %-72s VGPRs %3s scratch %s occupancy %s LDS %s\n", file, name, v, s, o, $(NF-1) }' "$TMP/$f.txt" |
    grep -E "clip_gemm_f32_kernel|compat_gemm_f32_kernel|lpips_conv3x3_relu_kernel|clip_layernorm_kernel|compat_ln_relu_kernel|lpips_finish_kernel"
  awk -v file="$f.hip" '
    /^_Z[A-Za-z0-9_]*:/ { name = $1; sub(":", "", name) }
    /v_mfma_/ { n[name]++ }
    END { for (k in n) printf "%-12s %-72s MFMA instructions %d\n", file, k, n[k] }' "$TMP/$f.s" | sort |
    grep -E "clip_gemm_f32_kernel|compat_gemm_f32_kernel|lpips_conv3x3_relu_kernel"
done
