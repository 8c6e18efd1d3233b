// The column-group linear map (groupops.hpp) for NL = 37 limbs.
#define BGN_NL 37
#include "group_impl.hpp"
