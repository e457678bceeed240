// aidax_mfmals2.hip — the two-layer instantiations of k_mfma_ls (aidax_mfmals.h), an object of their own: they are the longest
// compile of the tree, and a clean build should not wait for them behind the other forms.
#include "aidax_mfmals.h"

namespace aidax {

LpFn ls_fn_two_layers(int hidden, bool chain, int nprod)
{
    switch (hidden) {                                       // two layers: tiles started below
#define AIDAX_LS_CASE(HID) case HID: return ls_fn_for<HID, 2>(chain, nprod);
    AIDAX_LS_CASE(16) AIDAX_LS_CASE(32) AIDAX_LS_CASE(48) AIDAX_LS_CASE(64) AIDAX_LS_CASE(80) AIDAX_LS_CASE(96)
#undef AIDAX_LS_CASE
    default: return nullptr;
    }
}

}  // namespace aidax
