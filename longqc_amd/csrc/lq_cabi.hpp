// longqc_amd/csrc/lq_cabi.hpp -- the buffer-level C entry points without a handle (lqsdust_*, lqadapt_*): device selection, a
// stream for one call, and the mapping of exceptions to LQCOV_E_* codes -- by their type -- with the message in the caller's buffer.
#pragma once
#include "prim.hpp"
#include "../../include/lqcov.h"
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

// A file that cannot be opened, read or written, or whose content is not what its format says: LQCOV_E_IO, the whole message.
struct lq_io_error : std::runtime_error { using std::runtime_error::runtime_error; };
inline lq_io_error lq_open_error(const std::string &path, const std::string &what = std::string())
{
	return lq_io_error("failed to open file '" + path + "'" + (what.empty() ? what : ": " + what));
}
// What a byte source (bgzf.hpp, gzip.hpp, reader.cpp) finds wrong with its file's bytes or cannot read: it does not know the path, the
// reader catches this and throws lq_open_error(path, what()).  On its own it is any std::runtime_error.
struct lq_file_error : std::runtime_error { using std::runtime_error::runtime_error; };

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

// the stream of a call that has no handle to keep one in: the device selected, destroyed at the end of the scope
struct ScopedStream {
	hipStream_t s = nullptr;
	explicit ScopedStream(int device) { select_device(device); LQ_HIP_CHECK(hipStreamCreate(&s)); }
	~ScopedStream() { (void)hipStreamDestroy(s); }
	ScopedStream(const ScopedStream&) = delete; ScopedStream &operator=(const ScopedStream&) = delete;
	operator hipStream_t() const { return s; }
};

template <class F> int guarded(char *err, size_t errlen, F &&f)
{
	try { f(); return 0; }
	catch (const std::domain_error &e) { set_err(err, errlen, e.what()); return LQCOV_E_DOMAIN; }
	catch (const std::invalid_argument &e) { set_err(err, errlen, e.what()); return LQCOV_E_ARG; }
	catch (const lq_io_error &e) { set_err(err, errlen, e.what()); return LQCOV_E_IO; }
	catch (const std::runtime_error &e) { set_err(err, errlen, e.what()); return LQCOV_E_DEVICE; }
	catch (const std::exception &e) { set_err(err, errlen, e.what()); return LQCOV_E_STATE; }
}
} // namespace lq_cabi
