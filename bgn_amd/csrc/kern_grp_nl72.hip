// The column-group linear map (groupops.hpp) for NL = 72 limbs.
#define BGN_NL 72
#include "group_impl.hpp"
