#!/bin/bash
# Build libinstantir_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU).
set -e
cd "$(dirname "$0")"
OUT=../libinstantir_hip.so
FLAGS="--offload-arch=gfx950 -O3 -fPIC -std=c++17 -w"
mkdir -p build
pids=()
for f in gemm_conv gemm8 norm; do
  hipcc $FLAGS -c $f.hip -o build/$f.o &
  pids+=($!)
done
# attention: keep MFMA accumulators in VGPRs (softmax reads/rescales them every tile; AGPR form costs
# a v_accvgpr_read/write pair per touched element).  -fno-honor-nans: the row maxima are fmaxf over MFMA outputs; with NaNs
# honoured hipcc canonicalises every operand first (one extra v_max per score); -inf (masking) stays legal.
hipcc $FLAGS -mllvm -amdgpu-mfma-vgpr-form=1 -fno-honor-nans -c attention.hip -o build/attention.o &
pids+=($!)
hipcc $FLAGS -mllvm -amdgpu-mfma-vgpr-form=1 -fno-honor-nans -c attention_hd.hip -o build/attention_hd.o &
pids+=($!)
hipcc $FLAGS -mllvm -amdgpu-mfma-vgpr-form=1 -fno-honor-nans -c attention_1h.hip -o build/attention_1h.o &
pids+=($!)
hipcc $FLAGS -ffp-contract=off -c pointwise.hip -o build/pointwise.o &
pids+=($!)
hipcc $FLAGS -ffp-contract=off -c freeu.hip -o build/freeu.o &
pids+=($!)
hipcc $FLAGS -ffp-contract=off -c colorfix.hip -o build/colorfix.o &
pids+=($!)
hipcc $FLAGS -ffp-contract=off -c regionmap.hip -o build/regionmap.o &
pids+=($!)
hipcc $FLAGS -ffp-contract=off -c seg.hip -o build/seg.o &
pids+=($!)
hipcc $FLAGS -ffp-contract=off -c lqfidelity.hip -o build/lqfidelity.o &
pids+=($!)
hipcc $FLAGS -ffp-contract=off -c resample.hip -o build/resample.o &
pids+=($!)
hipcc $FLAGS -ffp-contract=off -c metrics.hip -o build/metrics.o &
pids+=($!)
hipcc $FLAGS -ffp-contract=off -c degrade.hip -o build/degrade.o &
pids+=($!)
hipcc $FLAGS -ffp-contract=off -c lpips.hip -o build/lpips.o &
pids+=($!)
hipcc $FLAGS -ffp-contract=off -c niqe.hip -o build/niqe.o &
pids+=($!)
hipcc $FLAGS -ffp-contract=off -c dists.hip -o build/dists.o &
pids+=($!)
for p in "${pids[@]}"; do wait $p; done
hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT build/gemm_conv.o build/gemm8.o build/attention.o build/attention_hd.o build/attention_1h.o build/norm.o build/pointwise.o build/freeu.o build/colorfix.o build/regionmap.o build/seg.o build/lqfidelity.o build/resample.o build/metrics.o build/degrade.o build/lpips.o build/niqe.o build/dists.o
echo "built $(realpath $OUT)"
