// szg_internal.hpp — what the translation units of libszg_hip.so share besides the public headers.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

struct szg_jpeg_frame; // szg/jpeg.h

namespace szg
{
// sets the calling thread's szg_last_error() text (defined in api_core.cpp)
void set_last_error(const char* message);
// why `frame` is not one szg/jpeg.h reconstructs: its geometry does not follow from its extent and sampling factors, or a
// coefficient pointer is NULL; "" when it is fine (defined in host_jpeg.cpp, shared by the host and the device entry points)
const char* jpeg_frame_problem(const struct ::szg_jpeg_frame& frame);
} // namespace szg
