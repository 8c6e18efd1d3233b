// The column-group linear map (groupops.hpp) for NL = 3 limbs.
#define BGN_NL 3
#include "group_impl.hpp"
