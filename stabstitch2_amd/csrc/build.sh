#!/bin/bash
# Build libstabstitch_hip.so for gfx950 (MI355X) in-tree.
#   stabstitch2_amd/csrc/build.sh           -> stabstitch2_amd/libstabstitch_hip.so         (the product)
#                                              stabstitch2_amd/libstabstitch_blend.so       (MULTIBAND fusion, blend.hip)
#                                              stabstitch2_amd/libstabstitch_seam.so        (MULTIBAND's DP seam, seam.hip)
#                                              stabstitch2_amd/libstabstitch_mbwarp.so      (MULTIBAND's direct warp, mbwarp.hip)
#                                              stabstitch2_amd/libstabstitch_surfaces.so    (NV12 surfaces -> BGR frames, surfaces.hip)
#                                              stabstitch2_amd/libstabstitch_smoothtail.so  (SmoothNet's clip-only Conv3d stack, smoothtail.hip)
#                                              stabstitch2_amd/libstabstitch_cover.so       (coverage bitmaps, largest covered rectangle, cover.hip)
#                                              stabstitch2_amd/libstabstitch_resample.so    (fixed-size antialiased output of a rectangle, resample.hip)
#   stabstitch2_amd/csrc/build.sh tuning    -> tools/libstabstitch_hip_tuning.so            (-DSS_TUNING: adds the
#       ss_debug_set / ss_debug_ptr knobs, the per-workgroup s_memtime stamps of tools/diag_*.py and the comparison kernels
#       that tests and tools/ab_*.py measure the product against; concluded experiments are not kept in it: LAB_NOTES.md,
#       "Retired experiment code")
# -ffp-contract=off: the samplers reproduce the reference's separate mul/add sequence (its out-of-range taps cancel
# exactly only without fma contraction); every intended fma is an explicit fmaf()/MFMA in the sources.
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
OUT="$HERE/../libstabstitch_hip.so"
DEFS=""
if [ "$1" = "tuning" ]; then
    OUT="$HERE/../../tools/libstabstitch_hip_tuning.so"
    DEFS="-DSS_TUNING"
fi
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -fvisibility=hidden"
"$HIPCC" $FLAGS $DEFS \
    "$HERE/conv.hip" "$HERE/wino.hip" "$HERE/corr.hip" "$HERE/geom.hip" "$HERE/render.hip" "$HERE/smooth.hip" "$HERE/metrics.hip" \
    "$HERE/frameio.hip" "$HERE/stem.hip" "$HERE/wino43.hip" \
    -o "$OUT"
echo "built $OUT"
if [ "$1" != "tuning" ]; then
    # every later feature is a library of its own (NAME.hip, include/stabstitch_NAME.h), so that the surface and the machine code of
    # libstabstitch_hip.so stay as they are
    for NAME in blend seam mbwarp surfaces smoothtail cover resample; do
        SIDE="$HERE/../libstabstitch_$NAME.so"
        "$HIPCC" $FLAGS "$HERE/$NAME.hip" -o "$SIDE"
        echo "built $SIDE"
    done
fi
