// The library's thread-local last-error string (gls_last_error): its setters, defined in gls_api.cpp.
#pragma once
int gls_internal_set_err(int code, const char *msg);
int gls_io_set_error(int code, const char *fmt, ...);
