#!/bin/bash
# Builds libhunter_hip.so (gfx950) in-tree.  hipcc cross-compiles without a GPU.
# The build FAILS if one of the hot kernels of the update (either WBC flavour included) spills to scratch memory: every scratch reload is followed by
# s_waitcnt vmcnt(0), which drains the software-pipelined record prefetch of the sweeps.
set -e
cd "$(dirname "$0")"
. ./hipcc_flags.sh
OUT=../libhunter_hip.so
# --ablate: the profiling variant with the phase-by-phase exits compiled in (tools/perf_quick.py --lib variants/libhunter_hip_ablate.so --ablate-lq)
# (the profiling variant may spill: its phase exits change the register allocation; scratch there is reported, not fatal)
ABLATE=0
if [ "$1" = "--ablate" ]; then shift; mkdir -p ../../variants; OUT=../../variants/libhunter_hip_ablate.so; ABLATE=1; set -- -DHB_ABLATE "$@"; fi
LOG=$(mktemp)
$HIPCC $HB_HIPCC_FLAGS -shared -Rpass-analysis=kernel-resource-usage -o $OUT hb_kernels.hip "$@" 2> "$LOG" || { cat "$LOG" >&2; rm -f "$LOG"; exit 1; }
grep -E "error|warning:" "$LOG" | grep -v "Wcomment" >&2 || true
python3 - "$LOG" "$ABLATE" <<'PY'
import re, sys
hot = ["k_lqE", "k_lq_tripE", "6k_gaitE", "8k_refgenE", "k_refgen_ikE", "k_refgen_nodesE", "k_estimatorE", "15k_refgen_groundE", "18k_estimator_groundE", "15k_refgen_gfieldE", "20k_refgen_ground_soleE", "20k_refgen_gfield_soleE", "18k_estimator_gfieldE", "k_warm_shiftE", "k_ric_bwdE", "k_ric_bwd4E", "k_ric_fwdE", "k_ric_fwd_wE", "5k_wbcE", "10k_wbc_certE", "6k_hwbcE", "11k_hwbc_certE", "k_ls_evalE", "k_ls_tail_evalE", "k_ls_eval_nodeE", "k_ls_tail_eval_nodeE", "k_ls_tail_decideE", "k_policy_evalE", "k_mpc_cert_nodesE", "k_mpc_cert_sweepE", "15k_plant_contactE", "14k_plant_jointsE", "14k_plant_hybridE", "22k_plant_contact_hybridE", "21k_plant_joints_hybridE", "15k_plant_terrainE", "22k_plant_terrain_jointsE", "22k_plant_terrain_hybridE", "29k_plant_terrain_joints_hybridE", "14k_plant_variedE", "21k_plant_varied_jointsE", "21k_plant_varied_hybridE", "28k_plant_varied_joints_hybridE", "15k_plant_profileE", "22k_plant_profile_jointsE", "22k_plant_profile_hybridE", "29k_plant_profile_joints_hybridE", "13k_plant_fieldE", "20k_plant_field_jointsE", "20k_plant_field_hybridE", "27k_plant_field_joints_hybridE", "15k_plant_episodeE", "15k_plant_respawnE", "21k_plant_respawn_fieldE", "18k_plant_field_drawE", "12k_plant_scanI", "20k_plant_profile_drawE", "16k_plant_scenarioE", "12k_plant_pushE"]
# the two-lane line-search kernels must leave room for a second wavefront on the SIMD: VGPR + AGPR <= 256
shared_simd = ["k_ls_evalE", "k_ls_tail_evalE"]
txt = open(sys.argv[1]).read()
rows, bad, fat = [], [], []
for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)", txt, re.S):
    name, vg, ag, scr, occ, lds = m.group(1), *map(int, m.groups()[1:])
    if any(h in name for h in hot):
        rows.append(f"  {name[:48]:48s} vgpr {vg:3d} agpr {ag:3d} scratch {scr:3d} B  waves/SIMD {occ}  lds {lds} B")
        if scr:
            bad.append(name)
        if any(h in name for h in shared_simd) and (vg + ag > 256 or occ < 2):
            fat.append(name)
print("hot-kernel resources (gfx950):")
print("\n".join(rows))
if bad and sys.argv[2] == "1":
    print("build.sh --ablate: scratch memory in " + ", ".join(bad) + " (profiling variant: tolerated)")
elif bad:
    sys.exit("build.sh: scratch memory in hot kernel(s): " + ", ".join(bad))
if fat and sys.argv[2] != "1":
    sys.exit("build.sh: more than 256 registers or fewer than two wavefronts per SIMD in " + ", ".join(fat))
PY
rm -f "$LOG"
# The device unit wrappers of the test suite (tests/gpu_unit/primitives.hip: one kernel per device-only primitive of hb_math.hpp /
# hb_tile.hpp / hb_qpfactor.hpp), same flags; built with the product so that it travels with the tree.  Not part of libhunter_hip.so.
if [ "$ABLATE" = "0" ] && [ -f ../../tests/gpu_unit/primitives.hip ]; then
  TMP=../../tests/gpu_unit/libhb_primitives.$$.so
  $HIPCC $HB_HIPCC_FLAGS -shared -o $TMP ../../tests/gpu_unit/primitives.hip || { rm -f $TMP; exit 1; }
  mv -f $TMP ../../tests/gpu_unit/libhb_primitives.so
fi
