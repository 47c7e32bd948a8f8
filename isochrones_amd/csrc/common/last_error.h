// A library's last error: the message its iso_<name>_last_error() returns, per thread, and the two ways an entry point
// sets it.  Internal and of internal linkage: each library that includes this has its own.
#ifndef ISO_COMMON_LAST_ERROR_H
#define ISO_COMMON_LAST_ERROR_H

#include <stdio.h>

namespace {

thread_local char g_err[256];

int fail(int rc, const char* msg) {
    snprintf(g_err, sizeof g_err, "%s", msg);
    return rc;
}

int fail(int rc, const char* who, const char* why) {            // "<entry point>: <what is wrong>"
    snprintf(g_err, sizeof g_err, "%s: %s", who, why);
    return rc;
}

}  // namespace

#endif
