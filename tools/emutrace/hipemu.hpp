// tools/emutrace/hipemu.hpp -- the test emulator's HIP stand-in with every launch named on stderr, in the words of the device build
// (lq_common.hpp, LQCOV_TRACE_LAUNCHES=1), so that two builds' launch orders compare without a GPU (tools/launch_order.py):
//   make -C longqc_amd/csrc emu EMUDIR=../../tools/emutrace      -> tools/emutrace/liblqcov_emu.so
#pragma once
#include "../../tests/emu/hipemu.hpp"
inline const bool emu_trace_launches = getenv("LQCOV_TRACE_LAUNCHES") && atoi(getenv("LQCOV_TRACE_LAUNCHES")) != 0;
#undef LQ_LAUNCH
#define LQ_LAUNCH(kern, grid, block, stream, ...) do { g_emu_kernel = #kern; \
		if (emu_trace_launches) { fprintf(stderr, "[lqcov] launch %s grid %u stream %p\n", #kern, (unsigned)dim3(grid).x, (void*)(stream)); fflush(stderr); } \
		emu_launch(kern, dim3(grid), dim3(block), __VA_ARGS__); } while (0)
