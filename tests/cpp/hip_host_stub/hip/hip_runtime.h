#include "hip_runtime_api.h"
