// sweep.hpp — the host side of a whole-device sweep, shared by the coverage
// checks (cu, mx, valu: one table entry per SIMD) and the LDS check (one per
// CU): device selection, the bounded relaunch until every unit has been seen,
// and the per-unit result dicts.  The counting itself is cov_tally in
// validator_problems.hpp; the kernels' frame is described on cu_coverage_kernel.

#pragma once

#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "hip_util.hpp"
#include "validator_problems.hpp"

namespace py = pybind11;

constexpr int kCovLdsWords = 16384;         // 64 KiB static LDS per workgroup
constexpr int kCovBlock = 256;              // one wave per SIMD, normally
constexpr int kCovBlocksPerCu = 2;          // floor(160 KiB / 64 KiB)

// s_getreg simm16 = id | offset << 6 | (size - 1) << 11; full 32 bits of each.
constexpr int kCovHwRegHwId = 4 | (31 << 11);
constexpr int kCovHwRegXccId = 20 | (31 << 11);

// Selects the device; its properties, once the CU count is a plausible one.
static hipDeviceProp_t select_device(const std::string& who, int device) {
  hipDeviceProp_t prop;
  HIP_CHECK(hipSetDevice(device));
  HIP_CHECK(hipGetDeviceProperties(&prop, device));
  if (prop.multiProcessorCount < 1 || prop.multiProcessorCount > kCovKeys)
    throw std::runtime_error(who + ": implausible compute unit count");
  return prop;
}

// The same for a coverage sweep, whose kernel claims 64 KiB of LDS; the CUs.
static int cov_select_device(const std::string& who, int device) {
  const hipDeviceProp_t prop = select_device(who, device);
  if (prop.sharedMemPerBlock < sizeof(uint32_t) * kCovLdsWords)
    throw std::runtime_error(
        who + ": device grants less than 64 KiB of LDS per workgroup");
  return prop.multiProcessorCount;
}

struct SweepRun {
  int cus = 0, rounds = 0;
  double elapsed_ms = 0.0;
  CovTally tally;
};

// `launch(round)` enqueues one round on the null stream; after each round the
// planes (see cov_tally) are downloaded and recounted, until the tally is
// complete or max_rounds rounds have run.
template <typename Launch>
static SweepRun sweep_relaunch(int cus, int simds, int max_rounds,
                               const DeviceBuf<uint32_t>& d_planes, Launch launch) {
  EventTimer timer;
  std::vector<uint32_t> h(d_planes.size());
  SweepRun run;
  run.cus = cus;
  while (run.rounds < max_rounds) {
    run.elapsed_ms += timer.time_ms([&] {
      launch(run.rounds);
      HIP_CHECK(hipGetLastError());
    });
    ++run.rounds;
    d_planes.download(h.data(), h.size());
    run.tally = cov_tally(h.data(), cus, simds);
    if (run.tally.complete) break;
  }
  return run;
}

// argument validation of a coverage sweep: before the first HIP call
static void cov_validate(const std::string& who, int reps, int max_rounds,
                         int poison_key, unsigned poison_mask, int mask_bits) {
  require_range(who, "reps", reps, 1, 4096);
  require_range(who, "max_rounds", max_rounds, 1, 64);
  require_poison_key(who, poison_key);
  if (poison_mask >= (1u << mask_bits))
    throw std::invalid_argument(who + ": poison_mask has " +
                                std::to_string(mask_bits) + " bits");
}

// A coverage sweep on the selected device: table upload and bounded relaunch.
// `launch(round, tab, slots)` enqueues the sweep's kernel on a grid of
// kCovBlocksPerCu x CUs workgroups.
template <typename Launch>
static SweepRun cov_run_sweep(int cus, int max_rounds,
                              const std::vector<uint32_t>& tab, Launch launch) {
  DeviceBuf<uint32_t> d_tab(tab.size());
  DeviceBuf<uint32_t> d_slots((size_t)4 * kCovSlots);  // waves | fail | hw_id | xcc_id
  d_tab.upload(tab.data(), tab.size());
  d_slots.fill(0);
  return sweep_relaunch(cus, 4, max_rounds, d_slots, [&](int round) {
    launch(round, d_tab.get(), d_slots.get());
  });
}

// per SIMD a unit has "simd" and "waves", per CU it has "workgroups"
static py::list sweep_unit_list(const CovTally& t, bool per_simd) {
  py::list units;
  for (const CovUnit& c : t.units) {
    py::dict u;
    u["key"] = c.key;
    u["xcc"] = c.key >> 8;
    u["hw_bits"] = c.key & 0xFF;
    if (per_simd) u["simd"] = c.simd;
    u[per_simd ? "waves" : "workgroups"] = c.waves;
    u["fail_mask"] = c.fail_mask;
    u["hw_id_raw"] = c.hw_id_raw;
    u["xcc_id_raw"] = c.xcc_id_raw;
    units.append(u);
  }
  return units;
}

static py::dict cov_sweep_dict(const SweepRun& run) {
  py::dict out;
  out["compute_units"] = run.cus;
  out["cus_covered"] = run.tally.cus_covered;
  out["simd_slots_covered"] = run.tally.slots_covered;
  out["waves_run"] = run.tally.waves_run;
  out["rounds"] = run.rounds;
  out["failed_slots"] = run.tally.failed_slots;
  out["units"] = sweep_unit_list(run.tally, true);
  out["elapsed_ms"] = run.elapsed_ms;
  return out;
}
