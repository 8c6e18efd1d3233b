// The column-group linear map (groupops.hpp) for NL = 36 limbs.
#define BGN_NL 36
#include "group_impl.hpp"
