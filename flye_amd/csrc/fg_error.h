// What the library throws inside and the C ABI turns into a code and fg_last_error's text.  Needs no HIP.
#pragma once
#include <string>

struct FgError { int code; std::string msg; };

// the text of the calling thread's last failed call that has no context (fg_paf_parse); fg_last_error(NULL) returns it
inline std::string& fgHostError()
{
	static thread_local std::string text;
	return text;
}
