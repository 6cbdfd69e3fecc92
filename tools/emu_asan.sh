#!/bin/bash
# The emulator build of the kernels (tests/emu) under AddressSanitizer: every out-of-bounds access of a kernel to a "device"
# buffer (heap) or to LDS (static arrays) stops the run with a report.  No GPU needed.
#   bash tools/emu_asan.sh [pytest args, default: the whole emulator suite]
cd "$(dirname "$0")/.."
OUT=${TMPDIR:-/tmp}/liblqcov_emu_asan.so
SRCS="engine.cpp api.cpp dust.cpp adapt.cpp gc.cpp chunk.cpp reader.cpp writer.cpp"      # (longqc_amd/csrc/Makefile's SRCS)
( cd longqc_amd/csrc && g++ -DLQ_EMU -include ../../tests/emu/hipemu.hpp -DLQ_EXACT_ALLOC -O1 -g -fsanitize=address -fno-omit-frame-pointer -std=c++17 -fPIC \
    -Wno-unused-function -Wno-unknown-pragmas $SRCS -shared -o "$OUT" -lz ) || exit 1
# (libstdc++ preloaded too: the sanitizer's __cxa_throw interceptor needs it at start-up, and the tests of refused inputs throw;
# what the environment preloads already stays, behind the sanitizer)
LQCOV_EMU_LIB="$OUT" LD_PRELOAD="$(gcc -print-file-name=libasan.so) $(gcc -print-file-name=libstdc++.so)${LD_PRELOAD:+ $LD_PRELOAD}" ASAN_OPTIONS=detect_leaks=0 \
  python -m pytest tests/test_emu_pipeline.py tests/test_mmi.py tests/test_sdust.py tests/test_adapter.py tests/test_gcfrac.py tests/test_chunkpass.py \
    tests/test_launch_caps.py tests/test_filechunks.py tests/test_inflate.py tests/test_inflate_caps.py tests/test_gzip_inflate.py tests/test_gzip_reader.py tests/test_gzip_caps.py -m "not gpu" -x -q "${@:--n 6}"
