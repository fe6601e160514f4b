// dab_internal.h — the error reporting every file of the library shares, the plain C++ ones
// included (not part of the ABI). The handle and what its host files share: dab_handle.h.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/dab.h"

namespace dab {

// Thread-local last error (dab_last_error). Returns `code` for `return set_error(...)`.
int set_error(int code, const std::string& msg);
void clear_error();

}  // namespace dab
