#!/bin/bash
# Timing-only calibration builds of the product walk (round 3, profiles/r03_calibration/): apply a
# temporary patch to the device headers, build lib/variants/libkhbsgs_<name>.so, restore the source.
#   pad_patch.py: after every field multiply, KHB_PAD_N instructions of kind KHB_PAD_OP
#                 (1 v_mov, 2 v_add_u32, 3 v_add_co, 4 v_addc, 5 mad->vcc, 6 mad->sgpr, 7 v_mul_lo,
#                 8 s_nop, 9 v_add3) in 4 independent chains; KHB_PAD_OP=0 is the barrier-only control.
#   nonop_patch.py: the carry-hazard s_nop pads removed (timing only).
#   block_patch.py: KHB_BLOCK threads per workgroup.
#   scr_patch.py: KHB_SCR_MASK=m keeps the prefix scratch in (i & m) entries per group (no HBM stream).
#   plainscr_patch.py: the prefix-scratch stream with plain loads and stores (the product's are non-temporal).
#   (round 5's half_patch.py is now the build define KHB_HALF_STREAM in device/scan_args.hpp: build_variant.sh half -DKHB_HALF_STREAM=1.)
#   scrplain_patch.py: scr_patch with plain accesses (the stream cache-resident; scr2plain / scr1plain, round 5).
#   scrhalf_patch.py: scrplain for the half prefix stream (round 6).
# The patches edit device/fe_asm.hpp (pad, nonop), device/scan_args.hpp (block) or device/walk.hpp (scr*, plainscr).
# Usage: tools/experiments/calib_build.sh pad|nonop|block|scr|plainscr|scrplain|scrhalf <name> [-DKEY=VAL ...]
set -e
KIND=$1; NAME=$2; shift 2
D=keyhuntm1cpu_amd/csrc/device
SRCS="fe_asm.hpp scan_args.hpp walk.hpp"
for f in $SRCS; do cp $D/$f /tmp/calib_$f; done
trap 'for f in $SRCS; do cp /tmp/calib_$f $D/$f; done' EXIT
python3 tools/experiments/${KIND}_patch.py
tools/build_variant.sh $NAME "$@"
