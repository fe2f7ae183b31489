// Shared by the C flattenings (host/*_capi.cpp): the error string behind each file's lvh_X_last_error, the guard that
// turns a C++ exception into a status code, and the "set the text, return the code" of an argument check.  Everything is
// in an anonymous namespace, so every translation unit that includes this header has an error string of its own:
// lvh_pgo_last_error() reports pgo's errors only.  Not part of any exported interface; include it from a .cpp only.
#pragma once
#include <exception>
#include <string>

#include "lvi_host.hpp"

namespace {
thread_local std::string g_err;

template <class F> int32_t guarded(F&& f)
{
    try { return f(); }
    catch (const lvi_host::Error& e) { g_err = e.what(); return e.code; }
    catch (const std::exception& e) { g_err = e.what(); return LVI_ERR_HIP; }
}

inline int32_t fail(const char* text, int32_t code = LVI_ERR_INVALID_ARG) { g_err = text; return code; }
}  // namespace
