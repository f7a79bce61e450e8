// Error messages of the C ABIs, shared by every library (each translation unit gets its own copy:
// the names are in an anonymous namespace).  Every failing call stores its message in the handle
// it was called on (kwk_last_error(eng), kwk_emit_last_error(em), ...), so a caller that moves
// between OS threads (a cgo goroutine) reads the message of its own handle's call; calls without a
// handle (kwk_engine_create, pinned host buffers) leave it in the calling thread's slot
// (kwk_last_error(NULL)).
#pragma once

#include <string>

#include "../../include/kwok_engine.h"

namespace {

thread_local std::string g_err;                 // the calling thread's slot
thread_local std::string* tl_err = nullptr;     // the handle's slot of the API call running on this thread

struct ErrScope {  // marks the handle's message an API call fills, for fail()
  std::string* prev;
  explicit ErrScope(std::string* target) : prev(tl_err) { tl_err = target; }
  ~ErrScope() { tl_err = prev; }
};

kwk_status fail(kwk_status code, const std::string& msg) {
  g_err = msg;
  if (tl_err) *tl_err = msg;
  return code;
}

}  // namespace

#ifdef __HIPCC__
#define HIP_TRY(x)                                                                                \
  do {                                                                                            \
    hipError_t e_ = (x);                                                                          \
    if (e_ != hipSuccess) return fail(KWK_EHIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)
#endif
