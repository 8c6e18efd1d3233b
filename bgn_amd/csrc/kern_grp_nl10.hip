// The column-group linear map (groupops.hpp) for NL = 10 limbs.
#define BGN_NL 10
#include "group_impl.hpp"
