// ZIP directory locator (zip_dir.cc): where one entry of a ZIP container lies, from the container's last bytes, its central
// directory and the entry's local header.  Plain C++, no HIP call, no I/O, no allocation: pure functions over caller buffers,
// every read bounds-checked.  The functions and their result type are part of the host ABI (include/znippy_host.h).
#pragma once
#include "../../../include/znippy_hip.h"
#include "../../../include/znippy_host.h"

// how much of a file's end znippy_zip_end_of_directory wants to see: the 22-byte record behind a comment of up to 65,535 bytes
#define ZN_ZIP_TAIL_MAX 65557u
