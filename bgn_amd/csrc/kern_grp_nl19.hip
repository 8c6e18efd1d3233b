// The column-group linear map (groupops.hpp) for NL = 19 limbs.
#define BGN_NL 19
#include "group_impl.hpp"
