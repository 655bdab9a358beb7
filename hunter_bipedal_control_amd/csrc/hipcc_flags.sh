# The device compile flags of libhunter_hip.so, sourced by csrc/build.sh and by the tools that inspect the shipped ISA
# (tools/asm_count.sh, tools/isa_vmseq.sh), so that what they count is what is built.
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
HB_HIPCC_FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -mllvm -disable-machine-licm -fPIC"
