// The strip build of the one-launch canonical objective node, gram_mid_kernel<true, true, true> (gram_mid.hip: mid_strips), in a
// translation unit of its own: the device code of gram_mid.hip and the one launch, nothing of its host part.  Kept apart so that the
// builds without strips stay the kernels they were, instruction for instruction (see the note in front of launch_gram_mid_strips there).
#define PMT_MID_STRIPS_TU 1
#include "gram_mid.hip"
