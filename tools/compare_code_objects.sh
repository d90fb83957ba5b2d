#!/bin/bash
# Byte compare of the gfx950 code objects of two builds' objects (variant_<mask>.o, heavy_<mask>.o, lrhip_<unit>.o): a change to the host side --
# the launch thunks of megapath_variant.hip / heavy_variant.hip, the sources behind include/lrhip.h -- must leave every kernel untouched.
#   tools/compare_code_objects.sh <obj dir of the parent build> <obj dir of this build>  >  profiles/<change>_code_objects.txt
# Prints one row per object (sha256 prefix of each side's code object, its size) and exits non-zero if any differs.  An object that holds
# no device code on either side (a host-only unit) is "no kernels", and differs from nothing.
BIN=${ROCM_PATH:-/opt/rocm}/lib/llvm/bin
# <object>: "<sha256 prefix> <bytes>" of its gfx950 code object
code_object() {
    local t; t=$(mktemp -d)
    if $BIN/llvm-objcopy --dump-section .hip_fatbin=$t/fatbin "$1" /dev/null 2>/dev/null &&
       $BIN/clang-offload-bundler --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=$t/fatbin --output=$t/co 2>/dev/null; then
        echo "$(sha256sum < $t/co | cut -c1-16) $(stat -c %s $t/co)"
    else
        echo "none 0"
    fi
    rm -rf "$t"
}
[ -d "$1" ] && [ -d "$2" ] || { echo "usage: $0 <parent obj dir> <obj dir>" >&2; exit 2; }
printf "%-14s %-18s %-18s %10s  %s\n" object parent this bytes verdict
same=0; different=0
for f in $(ls "$1" "$2" | grep -E '^((variant|heavy)_[0-9]+|lrhip_[a-z_]+)\.o$' | sort -u | sort -t_ -k1,1 -k2,2n); do
    a=($(code_object "$1/$f")); b=($(code_object "$2/$f"))
    if [ "${a[0]}" == "${b[0]}" ] && [ "${a[0]}" != none ]; then verdict=identical; same=$((same + 1))
    elif [ "${a[0]}" == none ] && [ "${b[0]}" == none ] && [[ $f == lrhip_* ]]; then verdict="no kernels"
    else verdict=DIFFERENT; different=$((different + 1)); fi
    printf "%-14s %-18s %-18s %10s  %s\n" "${f%.o}" "${a[0]}" "${b[0]}" "${b[1]}" "$verdict"
done
echo "identical $same, different $different"
[ $different == 0 ]
