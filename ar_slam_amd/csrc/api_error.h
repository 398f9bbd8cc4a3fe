// api_error.h -- errors behind the C-ABIs: an exception that carries its
// C-ABI code, and the guard that turns what an entry point throws into that
// code and the text of arslam_lm_last_error().
#pragma once

#include "arslam_lm.h"

#include <new>
#include <stdexcept>
#include <string>

namespace arslam {

// An error with the C-ABI code it maps to.
struct ApiError : std::runtime_error {
  int code;
  ApiError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

// message returned by arslam_lm_last_error() on the calling thread
void set_last_error(const std::string &msg);

inline void api_check(bool ok, int code, const char *msg) {
  if (!ok) throw ApiError(code, msg);
}

// The C boundary of the HIP library's entry points: runs f and turns what it
// throws into the C-ABI code, leaving the text for arslam_lm_last_error().
template <class F>
int api_guarded(F &&f) {
  try {
    f();
    return ARSLAM_OK;
  } catch (const ApiError &e) {
    set_last_error(e.what());
    return e.code;
  } catch (const std::bad_alloc &) {
    set_last_error("host out of memory");
    return ARSLAM_E_OUT_OF_MEMORY;
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return ARSLAM_E_HIP;
  } catch (...) {
    set_last_error("unknown error");
    return ARSLAM_E_HIP;
  }
}

}  // namespace arslam
