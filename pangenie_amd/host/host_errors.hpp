// host_errors.hpp — how pangenie_host.cpp and cohort.cpp report a refusal: std::runtime_error with the text of the reference's
// message or of the C ABI's error buffer.  Internal to pangenie_amd/host; not part of the public interface.
#pragma once
#include <stdexcept>
#include <string>

#include "../../include/pangenie_hmm.h"

namespace pangenie {

[[noreturn]] inline void fail(const std::string& msg) { throw std::runtime_error(msg); }
inline void check_rc(int rc, const char* err) {
    if (rc != PG_OK) fail(err && err[0] ? std::string(err) : ("pangenie_hmm error " + std::to_string(rc)));
}

}  // namespace pangenie
