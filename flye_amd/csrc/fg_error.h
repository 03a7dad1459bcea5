// What the library throws inside and the C ABI turns into a code and fg_last_error's text.  Needs no HIP.
#pragma once
#include <string>

struct FgError { int code; std::string msg; };
