// Launchers of the wide loss family (loss_wide.hip, 5 <= C <= 16); loss.hip checks the arguments and dispatches here.
#pragma once
#include "common.h"

int hpfg_loss_wide_partials(const HpfgLossArgs* a, const HpfgPeerX* px /* or NULL */, int nblk, void* stream);      // partial sums + reduction -> a->sums
int hpfg_loss_wide_finalize(const HpfgLossArgs* a, void* stream);
int hpfg_loss_wide_bwd(const HpfgLossArgs* a, const float* grad_scale_dev, int nblk, void* stream);
