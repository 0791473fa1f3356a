// stand-in for the HIP runtime header when a kernel file is compiled for the host (scripts/native/analysis_kernel_host.cpp)
#pragma once
