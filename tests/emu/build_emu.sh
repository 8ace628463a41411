#!/usr/bin/env bash
# Build the HOST-EMULATED device library (test infrastructure only; see hip/hip_runtime.h).
# usage: build_emu.sh                     -> libcfhip_emu.so
#        build_emu.sh NAME [-DFLAG ...]   -> libcfhip_emu_NAME.so: the same sources with extra defines (the diagnostic builds of
#                                            cf_dist.hip and cf_count2.hip, tests/test_emu_variants.py)
# Objects are kept in obj/ under a hash of the preprocessed source and the flags, so a build compiles only the sources whose
# preprocessed text differs from one built before (a variant of cf_dist.hip: that file alone, ~9 s).
set -euo pipefail
here="$(cd "$(dirname "$0")" && pwd)"
root="$(cd "$here/../.." && pwd)"
out="$here/libcfhip_emu.so"
san=()
opt=(-O2)
# CF_EMU_UBSAN=1: the same sources with UndefinedBehaviorSanitizer (tests/test_emu_ubsan.py) -> libcfhip_emu_ubsan.so
if [[ "${CF_EMU_UBSAN:-0}" == 1 ]]; then out="$here/libcfhip_emu_ubsan.so"; san=(-fsanitize=undefined -fno-sanitize-recover=undefined -fno-sanitize=alignment); opt=(-O1); fi
defs=()
if [[ $# -gt 0 ]]; then
    [[ "$1" =~ ^[A-Za-z0-9_]+$ ]] || { echo "build_emu.sh: bad build name '$1'" >&2; exit 2; }
    out="$here/libcfhip_emu_$1.so"; shift
    for d in "$@"; do [[ "$d" == -D* ]] || { echo "build_emu.sh: only -D flags follow the name, got '$d'" >&2; exit 2; }; defs+=("$d"); done
fi
flags=("${opt[@]}" "${san[@]}" -g -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-sign-compare -Wno-attributes
       -I"$here" -I"$root/include" -I"$root/centroflye_amd/csrc/hip")
# every kernel source except the RCCL transport; its place is taken by the file-based transport of the emulator
srcs=()
for f in "$root"/centroflye_amd/csrc/hip/*.hip; do [[ "$(basename "$f")" == cf_comm_rccl.hip ]] || srcs+=("$f"); done
srcs+=("$here/cfemu_runtime.cpp" "$here/cf_comm_emu.cpp")
cache="$here/obj"; mkdir -p "$cache"
objs=(); todo=()
for f in "${srcs[@]}"; do
    # (the extra defines are not part of the key themselves: a source they do not reach keeps the default build's object)
    key=$({ printf '%s\n' "${flags[@]}"; g++ "${flags[@]}" "${defs[@]}" -E -x c++ "$f"; } | sha1sum | cut -c1-16)
    o="$cache/$(basename "$f").$key.o"
    objs+=("$o")
    [[ -f "$o" ]] || todo+=("$f|$o")
done
# one compiler process per source that has no object yet (the kernels of cf_dist.hip alone are a third of the build)
jobs=$(nproc); (( jobs <= 16 )) || jobs=16
if (( ${#todo[@]} )); then
    printf '%s\n' "${todo[@]}" | xargs -P "$jobs" -I{} bash -c 's="${0%%|*}"; o="${0#*|}"; g++ "$@" -c -x c++ "$s" -o "$o.tmp$$" && mv "$o.tmp$$" "$o"' {} "${flags[@]}" "${defs[@]}"
fi
# relink only when the set of objects changed
stamp="$cache/$(basename "$out").objs"
list=$(printf '%s\n' "${objs[@]}")
if [[ -f "$out" && -f "$stamp" && "$(cat "$stamp")" == "$list" ]]; then exit 0; fi
g++ "${san[@]}" -shared -o "$out.tmp$$" "${objs[@]}"
mv "$out.tmp$$" "$out"
printf '%s\n' "$list" > "$stamp"
