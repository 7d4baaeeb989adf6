// host_gtab.h — TEST-ONLY: the fixed-base table of G for the CPU harnesses of the signing side, built on first use.  One harness is
// one translation unit, so the table is a static of the including file.  The includer defines IBFT_GTAB_BITS first (a small table:
// see recover_dev.h); the table's shape and gtab_entry come from recover_dev.h, included here under that setting.
#pragma once
#include <stdint.h>

#include <vector>

#include "recover_dev.h"

static std::vector<uint32_t> g_gtab;
static void gtab_init() {
  if (!g_gtab.empty()) return;
  g_gtab.resize((size_t)ibftk::GTAB_WINDOWS * ibftk::GTAB_ENTRIES * ibftk::GTAB_ENTRY_DWORDS);
  for (int t = 0; t < ibftk::GTAB_WINDOWS * ibftk::GTAB_ENTRIES; t++)
    ibftk::gtab_entry(t / ibftk::GTAB_ENTRIES, t % ibftk::GTAB_ENTRIES, g_gtab.data() + ibftk::GTAB_ENTRY_DWORDS * t);
}
