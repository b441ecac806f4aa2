#!/bin/sh
# Lab build of the product GEMM (csrc/gemm8.hip + gemm.hip + gemm5.hip + runtime.hip) with per-workgroup timeline stamps:
# scripts/micro/libgemm_tl.so, driven by scripts/gemm_timeline.py.  Not part of librtv_hip.so.
# A/B: EXTRA=-DRTV_G8_MFMA16=0 OUT=libgemm_tl_m32.so build_gemm_timeline.sh ; GEMM_TL_LIB=scripts/micro/libgemm_tl_m32.so gemm_timeline.py
set -e
cd "$(dirname "$0")"
C=../../realtime_video_amd/csrc
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -DRTV_GEMM_TIMELINE -Wno-unused-value $EXTRA \
  $C/gemm8.hip $C/gemm.hip $C/gemm5.hip $C/runtime.hip -o ${OUT:-libgemm_tl.so}
