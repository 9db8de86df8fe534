#!/bin/bash
# dump the gfx950 ISA of one kernel: tools/isa.sh <mangled-name-regex> [file.hip]
# compiled with the flags of the Makefile's CXXFLAGS line (as tests/test_abi_cpu.py does), so the ISA is the library's
cd "$(dirname "$0")/../opencl_fft_amd/csrc" || exit 1
F=${2:-fft_kernels.hip}
FLAGS=$(sed -n 's/^CXXFLAGS *= *//p' Makefile | sed 's/\$(ARCH)/gfx950/')
[ -n "$FLAGS" ] || { echo "CXXFLAGS not found in the Makefile" >&2; exit 1; }
/opt/rocm/bin/hipcc $FLAGS -save-temps=obj -c $F -o /tmp/isa_tmp.o 2>/dev/null || exit 1
S=/tmp/$(basename $F .hip)-hip-amdgcn-amd-amdhsa-gfx950.s
awk "/^$1:/,/s_endpgm/" $S
