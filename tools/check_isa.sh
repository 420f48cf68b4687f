#!/bin/bash
# dev: counts the packed-f32 VALU instructions per translation unit as the Makefile compiles them, and the forms whose LOW result
# takes the HIGH dword of a source (op_sel:[..1..]) — the form that misbehaved beside bf16 MFMAs (csrc/Makefile).
# Expected: no such form anywhere.  Then the footprint of every kernel of the convolution / GEMM units and of the recurrent
# matrix-core units (registers, spills, scratch, static LDS, instruction counts per class): the table a refactor of conv_common.h /
# split_mma.h / split_rows32.h is compared on, before and after (profiles/conv_kernel_footprint.txt, recorded before the buffer_load
# column existed, profiles/recurrent_kernel_footprint.txt, and for the page post-processing units profiles/post_kernel_footprint.txt, and for the nearest-word lookup profiles/lexicon_nearest.txt).   bash tools/check_isa.sh [unit ...]   (CPU only, about a minute;
# units default to all)
R=$(cd "$(dirname "$0")/.." && pwd)
C=$R/manuscript_ocr_amd/csrc
NOPK=$(sed -n 's/^NOPK_OBJS = //p' $C/Makefile)
FOOTPRINT="conv_igemm conv_split conv_split_pp winograd attn_beam_mfma attn_beam_mfma_alpha attn_forced_mfma attn_lexicon_mfma attn_lm_mfma attn_general attn_general_forced attn_general_lexicon attn_general_lm bilstm_mfma east_post east_tail reading_order quad_crop lexicon_nearest"
T=$(mktemp -d)
trap 'rm -rf $T' EXIT
units="$*"
[ -n "$units" ] || units=$(cd $C && ls *.hip | sed 's/\.hip$//')
bad=0
for f in $units; do
  fl=""
  case " $NOPK " in *" $f.o "*) fl="-Xclang -target-feature -Xclang -packed-fp32-ops";; esac
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I$R/include $fl -S --cuda-device-only $C/$f.hip -o $T/$f.s 2>/dev/null
  n=$(grep -c 'v_pk_[a-z]*_f32' $T/$f.s); m=$(grep 'v_pk_[a-z]*_f32' $T/$f.s | grep -c 'op_sel:')
  echo "$f: packed f32 instructions $n, cross-dword low-result forms $m"
  bad=$((bad + m))
done
echo
echo "kernel footprint: vgpr agpr sgpr spill(vgpr+sgpr) scratch_bytes static_lds | v_mfma ds_read ds_write global_load global_store scratch_* s_barrier v_cvt_pk_bf16_f32 buffer_load"
for f in $FOOTPRINT; do
  [ -f $T/$f.s ] || continue
  awk -v unit=$f '
    /^[A-Za-z_][A-Za-z0-9_]*:[ \t]*; @/ { fn = $1; sub(/:$/, "", fn); infn = 1; split("", c); next }
    /^\.Lfunc_end/ { infn = 0; next }
    infn && /^[ \t]+v_mfma_/ { c["mfma"]++ }
    infn && /^[ \t]+ds_read/ { c["dsr"]++ }
    infn && /^[ \t]+ds_write/ { c["dsw"]++ }
    infn && /^[ \t]+global_load/ { c["gl"]++ }
    infn && /^[ \t]+global_store/ { c["gs"]++ }
    infn && /^[ \t]+scratch_/ { c["scr"]++ }
    infn && /^[ \t]+s_barrier/ { c["bar"]++ }
    infn && /^[ \t]+v_cvt_pk_bf16_f32/ { c["cvt"]++ }
    infn && /^[ \t]+buffer_load/ { c["bl"]++ }
    /^; TotalNumSgprs:/ { sg = $3 }
    /^; NumVgprs:/ { vg = $3 }
    /^; NumAgprs:/ { ag = $3 }
    /^; ScratchSize:/ { ss = $3 }
    /^; LDSByteSize:/ {
      reg[fn] = sprintf("%3d %3d %3d", vg, ag, sg); rest[fn] = sprintf("%4d %6d | %4d %4d %4d %4d %4d %4d %3d %3d %4d", ss, $3,
        c["mfma"], c["dsr"], c["dsw"], c["gl"], c["gs"], c["scr"], c["bar"], c["cvt"], c["bl"])
    }
    /^[ \t]+\.name:[ \t]+_Z/ { mn = $2 }
    /^[ \t]+\.sgpr_spill_count:/ { sp = $2 }
    /^[ \t]+\.vgpr_spill_count:/ { spill[mn] = sprintf("%d+%d", $2, sp) }
    END { for (k in reg) if (k in spill) printf "%s\t%s %5s %s\n", k, reg[k], spill[k], rest[k] }
  ' $T/$f.s | sort | while IFS=$'\t' read -r sym vals; do
    printf '%-11s %-74s %s\n' "$f" "$(echo $sym | sed 's/DF16b/u6__bf16/' | c++filt | sed 's/(anonymous namespace):://; s/^void //; s/(.*//')" "$vals"
  done
done
echo
[ $bad -eq 0 ] && echo "OK: no cross-dword low-result packed form" || { echo "FOUND $bad"; exit 1; }
