#!/bin/bash
# isa_diff.sh <rev> [jobs]
# Proves a source change leaves the emitted code alone: compiles every object the Makefile builds (and
# tools/mfma16_gemm_check.hip) to device and host assembly, once from <rev> and once from the working tree,
# with the Makefile's flags and defines, and diffs the two after dropping the per-translation-unit
# __hip_cuid_<hash> lines.  Device assembly must come out identical; host assembly may differ only in the
# __LINE__ / __FILE__ constants of the error-reporting macros, so its diffs are printed for reading.
# A source that only one of the two trees has is named and skipped.  Exits non-zero if any device assembly differs.  Needs no GPU.
set -eo pipefail
rev=${1:?usage: isa_diff.sh <rev> [jobs]}; jobs=${2:-8}
repo=$(cd "$(dirname "$0")/.." && pwd)
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
work=$(mktemp -d); trap '[ -n "$KEEP" ] || rm -rf "$work"' EXIT
mkdir -p "$work/old" "$work/new"
git -C "$repo" archive "$rev" early_exit_transformer_amd/csrc include tools/mfma16_gemm_check.hip | tar -x -C "$work/old"
mkdir -p "$work/new/early_exit_transformer_amd" "$work/new/tools"
cp -r "$repo/early_exit_transformer_amd/csrc" "$work/new/early_exit_transformer_amd/"
cp "$repo/tools/mfma16_gemm_check.hip" "$work/new/tools/"
cp -r "$repo/include" "$work/new/"

# object name, source (relative to csrc), extra flags: the Makefile's SRCS, then its extra objects of ffn.hip and the check program
objects() {
  for s in $(sed -n 's/^SRCS := //p' "$repo/early_exit_transformer_amd/csrc/Makefile"); do echo "${s%.hip} $s -fPIC"; done
  echo "ffn512 ffn.hip -fPIC -DEEC_FFN_D=512"
  echo "ffn_train ffn.hip -fPIC -DEEC_FFN_TRAIN"
  echo "ffn_train_bwd ffn.hip -fPIC -DEEC_FFN_TRAIN_BWD"
  echo "mfma16_gemm_check ../../tools/mfma16_gemm_check.hip -I."
}

compile() {  # <tree> <side> <obj> <src> <flags...>
  local tree=$1 side=$2 obj=$3 src=$4; shift 4
  cd "$work/$tree/early_exit_transformer_amd/csrc"
  [ -f "$src" ] || { : > "$work/$tree.$obj.$side.s"; return 0; }  # a source only one side has: reported as such below
  "$HIPCC" -O3 -std=c++17 --offload-arch=gfx950 -Wno-unused-function -Wno-pass-failed "$@" \
    --cuda-$side-only -S "$src" -o - 2>"$work/$tree.$obj.$side.err" | grep -v __hip_cuid_ > "$work/$tree.$obj.$side.s"
}
export -f compile; export work HIPCC repo

objects | while read -r obj src flags; do
  for tree in old new; do for side in device host; do echo "$tree $side $obj $src $flags"; done; done
done | xargs -P "$jobs" -L 1 bash -c 'compile "$@" || { echo "compile failed: $*" >&2; exit 255; }' _

status=0
while read -r obj src flags; do
  if [ ! -s "$work/old.$obj.device.s" ] || [ ! -s "$work/new.$obj.device.s" ]; then
    printf '%-18s only in one tree: nothing to compare\n' "$obj"; continue
  fi
  if cmp -s "$work/old.$obj.device.s" "$work/new.$obj.device.s"; then dev=same; else dev=DIFFERENT; status=1; fi
  hostn=$(diff "$work/old.$obj.host.s" "$work/new.$obj.host.s" | grep -c '^[<>]' || true)
  printf '%-18s device %-9s host: %s changed lines\n' "$obj" "$dev" "$hostn"
  [ "$dev" = same ] || { diff "$work/old.$obj.device.s" "$work/new.$obj.device.s" | head -40 || true; }
  [ "$hostn" = 0 ] || { diff "$work/old.$obj.host.s" "$work/new.$obj.host.s" | grep "^[<>]" | head -20 || true; }
done < <(objects)
exit $status
