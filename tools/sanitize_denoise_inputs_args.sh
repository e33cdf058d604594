#!/bin/bash
# CPU-only sanitizer run of the host code of the stage between the raw films and the denoiser (the argument checks and the parameter packing of
# dtof_denoise_inputs_async and the sigma_position formed from the extent words, csrc/dtof_denoise_inputs_args.h):
#   tools/sanitize_denoise_inputs_args.sh
# builds tests/dev/asan_denoise_inputs_args.cpp with -fsanitize=address,undefined (plain C++, no HIP, no GPU needed) and runs it.  Prints its count of accepted and
# refused argument sets; any sanitizer report or failed expectation ends it with a non-zero status.
set -eu
root=$(cd "$(dirname "$0")/.." && pwd)
work=$(mktemp -d /tmp/dtof_asan_denoise_inputs.XXXXXX)
${CXX:-/opt/rocm/lib/llvm/bin/clang++} -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -I"$root/mitsuba3dopplertof_amd/csrc" "$root/tests/dev/asan_denoise_inputs_args.cpp" -o "$work/denoise_inputs_args"
"$work/denoise_inputs_args"
rm -rf "$work"
