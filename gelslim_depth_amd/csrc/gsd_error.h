// gsd_error.h -- host-side error plumbing (thread-local message, defined in gsd_api.hip); needs no device.
#pragma once
void gsd_set_error(const char* fmt, ...);
#define GSD_REQUIRE(cond, code, ...)                 \
  do {                                               \
    if (!(cond)) {                                   \
      gsd_set_error(__VA_ARGS__);                    \
      return (code);                                 \
    }                                                \
  } while (0)
