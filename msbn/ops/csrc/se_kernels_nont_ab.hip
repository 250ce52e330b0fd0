// A/B build variant of se_kernels.hip with nontemporal accesses
// disabled (see bn_kernels_nont_ab.hip): own translation unit, own object.
#define MSBN_DISABLE_NT 1
#include "se_kernels.hip"
