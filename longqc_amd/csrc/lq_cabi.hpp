// longqc_amd/csrc/lq_cabi.hpp -- the buffer-level C entry points without a handle (lqsdust_*, lqadapt_*): device selection and
// the mapping of exceptions to LQCOV_E_* codes with the message in the caller's buffer.
#pragma once
#include "prim.hpp"
#include "../../include/lqcov.h"
#include <cstdio>
#include <cstring>
#include <stdexcept>

namespace lq_cabi {
inline void set_err(char *err, size_t n, const char *msg) { if (err && n) snprintf(err, n, "%s", msg); }

inline int select_device(int device)
{
	int nd = 0;
	if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) throw std::runtime_error("no HIP device available");
	if (device < 0 || device >= nd) throw std::runtime_error("HIP device index out of range");
	LQ_HIP_CHECK(hipSetDevice(device));
	return device;
}

template <class F> int guarded(char *err, size_t errlen, F &&f)
{
	try { f(); return 0; }
	catch (const std::domain_error &e) { set_err(err, errlen, e.what()); return LQCOV_E_DOMAIN; }
	catch (const std::invalid_argument &e) { set_err(err, errlen, e.what()); return LQCOV_E_ARG; }
	catch (const std::runtime_error &e) {
		set_err(err, errlen, e.what());
		return strstr(e.what(), "failed to open") ? LQCOV_E_IO : LQCOV_E_DEVICE;
	}
	catch (const std::exception &e) { set_err(err, errlen, e.what()); return LQCOV_E_STATE; }
}
} // namespace lq_cabi
