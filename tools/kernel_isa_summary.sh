#!/bin/bash
# One line per kernel of a translation unit of diff_unet_amos_amd/csrc, from the gfx950 assembly hipcc emits with the
# Makefile's own flags (make print-cxxflags): register counts, scratch, static LDS, occupancy, code length and the number of
# MFMA, ds_read_b128, global load, global store, s_barrier and s_waitcnt instructions.  Two such summaries (before / after a
# change that must not move the kernels) are compared with diff; only `code` may differ.
#   tools/kernel_isa_summary.sh <file.hip> [extra hipcc flags]
set -e -o pipefail
src=$1; shift
csrc=$(cd "$(dirname "$0")/../diff_unet_amos_amd/csrc" && pwd)
flags=$(make -s --no-print-directory -C "$csrc" print-cxxflags)
hipcc=$(make -s --no-print-directory -C "$csrc" print-hipcc)
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
"$hipcc" $flags "$@" -Wno-unused-command-line-argument -S --cuda-device-only "$src" -o "$tmp/k.s"
awk -v file="$(basename "$src")" '
  function count(re) { if ($0 ~ re) n[re]++ }
  /^_Z[A-Za-z0-9_]+:/ { fn = $1; sub(/:$/, "", fn); delete n; body = 1; next }
  /^\.Lfunc_end/ { body = 0 }
  body && /^\t[a-z]/ {
    count("^\tv_mfma"); count("^\tds_read_b128"); count("^\tglobal_load"); count("^\tglobal_store")
    count("^\ts_barrier"); count("^\ts_waitcnt")
  }
  fn != "" && /^; codeLenInByte = / { code = $4 }
  fn != "" && /^; TotalNumSgprs: / { sgpr = $3 }
  fn != "" && /^; TotalNumVgprs: / { vgpr = $3 }
  fn != "" && /^; ScratchSize: / { scratch = $3 }
  fn != "" && /^; LDSByteSize: / { lds = $3 }
  fn != "" && /^; Occupancy: / {
    occ = $3
    printf "%s %s vgpr=%d sgpr=%d scratch=%d lds=%d occ=%d mfma=%d ds_read_b128=%d gload=%d gstore=%d barrier=%d waitcnt=%d code=%d\n",
           file, fn, vgpr, sgpr, scratch, lds, occ, n["^\tv_mfma"], n["^\tds_read_b128"], n["^\tglobal_load"], n["^\tglobal_store"],
           n["^\ts_barrier"], n["^\ts_waitcnt"], code
    fn = ""
  }
' "$tmp/k.s" | sort
