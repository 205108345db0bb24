// host_place.h -- the search for a placement of x and v in HBM, and the allocation of the two; included by picstep.hip alone, in its
// anonymous namespace behind its helpers (nothing in here is part of the ABI: pic_placement_info and pic_placement_stats are)
#pragma once

// Where x and v land in HBM decides how fast they stream together.  On an unfragmented MI355X the 288 GiB behave as nine regions
// of 32 GiB: a kernel that streams two arrays lying in the SAME region runs at 5.25 TB/s, with the arrays in two DIFFERENT
// regions at 6.05 TB/s, whichever regions and whatever the access pattern (profiles/window_probe.hip: one 120 GiB block, x fixed,
// v moved through it; profiles/experiments_r2.md 15).  A fresh device hands out neighbouring memory, so x and v of a default
// allocation share a region almost always; on a device whose memory has been through other processes a block is a mixture of
// pages from several regions (profiles/touch_probe.hip, experiments_r4.md 1: the class of a 64 MB window follows the window of x
// it is paired with, not the candidate), which is why the search times WHOLE blocks, never windows of them.
// For particle states that live in HBM (>= 256 MB) x and v are therefore two allocations: x first, then blocks of the same
// size one after the other (they are laid down in sequence), and every 3 GiB the pair (x, newest block) is timed with a streaming
// pass.  The search is a policy on RATIOS, not on this part's numbers: it ends sixteen readings after the best pair seen streams
// >= 10 % faster than the slowest one seen (the kinds have been told apart and we hold a fast one; the best of all is kept), after
// 42 GiB walked without an improvement (more than a region, all pairs alike: nothing to gain on this device), or when a third of
// the free memory is held; everything but x and v is freed before the call returns.
// pic_config.placement = PIC_PLACE_OFF skips it (x | v in one block).  Smaller states keep x | v in one block too (they sit in
// the Infinity Cache, and the one-copy read-back of pic_get_particles wants them adjacent).
//
// Where the time goes, and why the search comes in LEGS of at most 100 ms (round 4, profiles/experiments_r4.md 1).
// * Nothing is paid for the first touch of a block (touch_probe: first pass 330 us, later ones 347): a candidate is not cleared
//   here, a reading is one timed pass behind one untimed pass.
// * What costs is hipMalloc of memory the device hands out for the first time since it came up: the driver clears it, 1.3 ms per
//   512 MB block with the GPU otherwise idle and 3-6 ms under a streaming kernel (released memory is wiped in the background and
//   comes back in 20-70 us; a hipMalloc right behind the exit of a process that held tens of gigabytes can also sit and wait for
//   that wipe, 0.6-1.5 s seen -- nothing a caller of hipMalloc can bound).  A first create on such a device has x at the very start
//   of a region, 31 GiB -- 80 to 200 ms of allocations -- from the first block that pairs well with it.  No budget that a
//   constructor may take covers that.  But what one
//   leg has cleared and given back stays clean, so the NEXT leg walks through it in microseconds per block and spends its 100 ms
//   beyond: pic_create runs the first leg, and while it ends for lack of time pic_reset / pic_reset_sampled -- which replace the
//   particles anyway, so that moving v costs nothing -- run further ones (at most kMaxLegs, and only as long as pic_device_ptrs has
//   not handed the addresses to anybody).
// * The blocks are allocated by a thread of the call's own while the calling thread times; over never-used memory (slow mallocs) the
//   two take turns instead, because the clear and the timed stream slow each other down.
// * A device that has rested >= 3 ms runs its next 10-20 ms 4-13 % slow (early_steps3.py), and readings taken at different points
//   of that ramp show a "10 % faster" pair of the SAME kind.  Every reading is therefore a RATIO: the time of (x, candidate) over
//   the time of (x, the leg's first block) taken in the same breath (again whenever the stream has rested since), behind a filler.
struct BlockFeed {                                  // candidate blocks, allocated by a thread of their own (placement_leg)
  std::mutex m;
  std::condition_variable cv;
  std::vector<void*> blocks;                        // in allocation order; only ever grown by the feeder
  size_t taken = 0;                                 // blocks.size() when the timing thread last took one
  size_t lead = 1;                                  // the feeder stays at most this many blocks ahead of `taken`
  bool stop = false, done = false;
  bool timing = false;                              // a reading is being taken
  bool slow = false;                                // the last hipMalloc was of never-used memory (being cleared): take turns with the readings
  double malloc_seconds = 0.0;
};

constexpr int kMaxLegs = 4;

// One leg of the search.  On entry h->x is allocated; h->v is the block kept so far, or null (first leg).
void placement_leg(pic_handle* h, size_t pbytes) {
  // Everything the search allocates has to be given back, and the driver wipes released memory before it hands it out again
  // (asynchronously; whatever allocates next on the device may wait for that): an untouched 32 GiB spacer that carried the search out
  // of x's own region at once made the next pic_create of a create / destroy loop take 0.4-3 s (experiments_r3.md 18).  Blocks of
  // the state's own size, given back within the call, do not.
  constexpr size_t kLead = (size_t)3 << 30;         // distance between two readings
  constexpr double kGain = 1.10;                    // slowest / best (normalised) at which the search has found what it looks for
  constexpr size_t kPatience = (size_t)42 << 30;    // walked without an improvement before giving up: more than the 32 GiB a region
                                                    // spans (15 GiB gave up inside x's own region on some boxes: 1049 instead of 958 us)
  constexpr int kMore = 16;                         // readings beyond the first that passes kGain
  // per leg, the release of the blocks included: 100 ms, or what forty steps of the handle being placed take if that is more (a
  // step moves 12 x pbytes at ~6 TB/s: 1 ms at config 2, 4 ms at config 4's share, 10 ms at config 5's -- whose 2-5 GB blocks cost
  // 5-60 ms each to allocate on a device that hands them out for the first time)
  const double kMaxSeconds = h->cfg.placement_ms > 0 ? 1e-3 * h->cfg.placement_ms : std::max(0.100, 40.0 * 12.0 * (double)pbytes / 6.0e12);
  constexpr double kFreeSeconds = 0.0002;           // what giving one block back costs (hipFree: 25 ms for 110 blocks)
  constexpr double kSlowPerGiB = 0.0008;            // a hipMalloc slower than this per GiB is clearing never-used memory
  constexpr int kMaxBlocks = 192;
  PlacementStats& st = h->place;
  PlacementState& ps = h->place_state;
  const auto t_begin = std::chrono::steady_clock::now();
  auto seconds = [t_begin]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count(); };
  ps.legs += 1;
  size_t free_b = 0, total_b = 0;
  EventOwner e0, e1;
  bool ok = hipMemGetInfo(&free_b, &total_b) == hipSuccess && (e0 = make_event()) && (e1 = make_event());
  const size_t budget = free_b / 3;
  const long long n2 = (long long)(pbytes / sizeof(double2));
  long long nb = n2 / ((long long)BLOCK * 8);
  if (nb < 256) nb = 256;
  const long long chunk2 = (n2 + nb - 1) / nb;
  const long long nbh = (nb + 1) / 2, chunk2h = (n2 / 2 + nbh - 1) / nbh;
  double2* xa = static_cast<double2*>(h->x.get());
  // filler: the two halves of x streamed against each other (the same kernel at half the size), ~0.1 ms per GB of state
  auto filler = [&](int passes) {
    for (int r = 0; r < passes; ++r)
      hipLaunchKernelGGL(stream_probe_kernel, dim3((unsigned)nbh), dim3(BLOCK), 0, h->stream, xa, xa + n2 / 2, n2 / 2, chunk2h, 1.0, r & 1);
  };
  const double pass_ms_guess = 2.0 * (double)pbytes / 5.0e9;           // one filler pass moves 2 x pbytes at ~5 TB/s
  const int fill_1ms = std::max(1, (int)std::ceil(1.0 / pass_ms_guess));
  auto pair_ms = [&](void* vb, float* ms) {                            // one untimed pass over (x, block), one timed
    double2* b = static_cast<double2*>(vb);
    hipLaunchKernelGGL(stream_probe_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, h->stream, xa, b, n2, chunk2, 1.0, 0);
    bool good = hipGetLastError() == hipSuccess && hipEventRecord(e0, h->stream) == hipSuccess;
    hipLaunchKernelGGL(stream_probe_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, h->stream, xa, b, n2, chunk2, 1.0, 0);
    return good && hipGetLastError() == hipSuccess && hipEventRecord(e1, h->stream) == hipSuccess &&
           hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(ms, e0, e1) == hipSuccess;
  };
  const double gb_per_ms = 4.0 * (double)pbytes / 1e6;                // one pass, 2 arrays read and written: GB/s = this / ms

  BlockFeed feed;
  const size_t lead_blocks = std::max<size_t>(1, kLead / pbytes);
  const int device = h->cfg.device_id;
  std::thread feeder;
  if (ok && !ps.x_cleared) {
    ok = hipMemsetAsync(h->x, 0, pbytes, h->stream) == hipSuccess;    // (x holds particles in a later leg: the passes scale by 1.0)
    ps.x_cleared = true;
  }
  if (ok) {
    feed.lead = lead_blocks;
    try {
    feeder = std::thread([&feed, seconds, pbytes, budget, device, kMaxSeconds]() {
      const bool dev_ok = hipSetDevice(device) == hipSuccess;
      for (;;) {
        {
          std::unique_lock<std::mutex> lk(feed.m);
          feed.cv.wait(lk, [&] { return feed.stop || (feed.blocks.size() < feed.taken + feed.lead && !(feed.slow && feed.timing)); });
          if (feed.stop || !dev_ok || (int)feed.blocks.size() >= kMaxBlocks || (feed.blocks.size() + 2) * pbytes > budget ||
              seconds() + kFreeSeconds * (double)feed.blocks.size() > kMaxSeconds)
            break;
        }
        void* b = nullptr;
        const double tm = seconds();
        const bool got = hipMalloc(&b, pbytes) == hipSuccess;
        const double dt = seconds() - tm;
        std::lock_guard<std::mutex> lk(feed.m);
        feed.malloc_seconds += dt;
        feed.slow = dt > kSlowPerGiB * ((double)pbytes / (double)(1ull << 30));
        if (!got) { (void)hipGetLastError(); break; }
        feed.blocks.push_back(b);
        feed.cv.notify_all();
      }
      std::lock_guard<std::mutex> lk(feed.m);
      feed.done = true;
      feed.cv.notify_all();
    });
    } catch (...) {                                                   // no thread to be had: no search
      ok = false;
    }
  }
  // normalised readings: time of (x, block) / time of (x, the leg's first block) taken in the same breath
  void* ref = nullptr;
  float ref_ms = 0.f;
  double last_reading_at = -1.0;                                      // seconds() when the stream last finished a reading
  auto reading = [&](void* b, double* norm, float* raw_ms) {
    const double t0 = seconds();
    {
      std::lock_guard<std::mutex> lk(feed.m);
      feed.timing = true;
    }
    bool good = true;
    const bool rested = last_reading_at < 0.0 || t0 - last_reading_at > 0.0005;
    if (rested) {                                                     // the reference again, behind a filler: same point of the ramp
      filler(last_reading_at < 0.0 ? 4 * fill_1ms : fill_1ms);
      good = pair_ms(ref, &ref_ms);
    }
    if (good && b != ref) good = pair_ms(b, raw_ms); else *raw_ms = ref_ms;
    last_reading_at = seconds();
    {
      std::lock_guard<std::mutex> lk(feed.m);
      feed.timing = false;
      feed.cv.notify_all();
    }
    *norm = (double)*raw_ms / (double)ref_ms;
    st.timing_seconds += seconds() - t0;
    return good;
  };
  void* best = h->v;                                                  // the block kept by earlier legs, or null
  double best_n = ps.best_n, worst_n = ps.worst_n;                    // normalised; 0 = none yet
  // raw ms of the kept pair's reading and of the slowest reading of the leg (the rates pic_placement reports).  Blocks are chosen on
  // normalised readings, whose raw times were taken against different references: the pair with the largest ratio can stream faster
  // than the one kept, so the slowest rate reported is that of the slowest raw reading, never above the kept pair's.
  float best_raw = 0.f, slowest_raw = 0.f;
  int timed = 0, found_at = 0;
  size_t last = 0, best_at = 0;                                       // blocks.size() at the last / at the best reading
  int outcome = PIC_PLACED_MEMORY;                                    // (the feeder ran into the block or memory limit, or hipMalloc failed)
  while (ok) {
    void* b = nullptr;
    {
      std::unique_lock<std::mutex> lk(feed.m);
      // the next reading is due `lead` blocks further on (or on what the feeder managed before it stopped)
      feed.cv.wait(lk, [&] { return feed.done || feed.blocks.size() >= last + feed.lead; });
      if (feed.blocks.size() == last) break;                          // the feeder has stopped and every block it made has been looked at
      last = feed.taken = feed.blocks.size();
      b = feed.blocks.back();
      if (found_at > 0) feed.lead = 1;                                // (past the first find every block is looked at: fewer to give back)
      if (!ref) ref = feed.blocks.front();
      feed.cv.notify_all();
    }
    if (seconds() + kFreeSeconds * (double)last > kMaxSeconds) {      // (the 100 ms include giving the blocks back)
      outcome = PIC_PLACED_TIMEOUT;
      break;
    }
    if (last <= ps.frontier) continue;                                // an earlier leg has been here: nothing new to learn
    double n = 0.0;
    float raw = 0.f;
    if (timed == 0) {
      // first reading of a leg: the reference itself (first leg: it is a candidate like any other, n = 1), or where the block
      // kept by the earlier legs stands today
      void* first = h->v ? h->v : ref;
      ok = reading(first, &n, &raw);
      if (!ok) break;
      best = first; best_n = n; best_raw = raw; best_at = last;
      if (worst_n < n) worst_n = n;
      slowest_raw = std::max(slowest_raw, raw);
      ++timed;
      if (b == first) continue;
    }
    ok = reading(b, &n, &raw);
    if (!ok) break;
    ++timed;
    if (best_n == 0.0 || n < best_n) { best = b; best_n = n; best_raw = raw; best_at = last; }
    if (n > worst_n) worst_n = n;
    slowest_raw = std::max(slowest_raw, raw);
    if (worst_n >= kGain * best_n) {                                  // a fast pair, known to be one ...
      // ... but there are more than two kinds (5.0-5.3 / 5.6-5.75 / 5.85-6.0 TB/s read on used devices, 0.983 / 0.970 / 0.963 ms per
      // step at config 2), and the first pair 10 % above the slowest is often of the middle one: a reading costs 0.7 ms, so
      // kMore further blocks are looked at and the best of all is kept
      if (found_at == 0) found_at = timed;
      if (timed - found_at >= kMore) { outcome = PIC_PLACED_FOUND; break; }
      continue;
    }
    // (for the 2-5 GB blocks of configs 4 and 5 that is sixteen blocks at least: nine alike have been followed by a fast one)
    if ((last - best_at) * pbytes >= kPatience && last - best_at >= 16) { outcome = PIC_PLACED_PATIENCE; break; }
  }
  if (feeder.joinable()) {
    {
      std::lock_guard<std::mutex> lk(feed.m);
      feed.stop = true;
      feed.cv.notify_all();
    }
    feeder.join();
  }
  if (outcome == PIC_PLACED_MEMORY && seconds() + kFreeSeconds * (double)feed.blocks.size() > kMaxSeconds)
    outcome = PIC_PLACED_TIMEOUT;                                     // (the feeder's own clock check)
  if (found_at > 0) outcome = PIC_PLACED_FOUND;                       // a fast pair is in hand: no further leg for the rest of the sixteen
  (void)hipStreamSynchronize(h->stream);
  e0.reset();                                                         // (the events go here, inside the leg's clock)
  e1.reset();
  (void)hipGetLastError();
  std::vector<void*>& blocks = feed.blocks;
  if (!best && !blocks.empty()) best = blocks.front();                // nothing could be timed: any block will do
  const double tf = seconds();
  for (void* b : blocks)
    if (b != best) hipFree(b);
  h->v_block.reset(best);                                             // (frees the block kept so far if a later leg found a better one)
  st.free_seconds += seconds() - tf;
  h->v = best;
  ps.best_n = best_n; ps.worst_n = worst_n;
  ps.found = found_at > 0;
  ps.frontier = std::max(ps.frontier, blocks.size());
  st.blocks += (int)blocks.size();
  st.pairs_timed += timed;
  st.malloc_seconds += feed.malloc_seconds;
  st.outcome = outcome;
  if (best_raw > 0.f) st.kept_gbytes_per_s = gb_per_ms / best_raw;
  if (slowest_raw > 0.f && (st.slowest_gbytes_per_s == 0.0 || gb_per_ms / slowest_raw < st.slowest_gbytes_per_s))
    st.slowest_gbytes_per_s = gb_per_ms / slowest_raw;
  st.seconds += seconds();
  st.legs = ps.legs;
}

hipError_t alloc_particles(pic_handle* h, size_t pbytes) {
  h->place = PlacementStats{};
  h->place_state = PlacementState{};
  if (!h->v_separate) {                                                // (host_plan.h: below 256 MB, or PIC_PLACE_OFF)
    const hipError_t e = alloc(h->x, 2 * pbytes);
    h->v = static_cast<char*>(h->x.get()) + pbytes;
    return e;
  }
  hipError_t e = alloc(h->x, pbytes);
  if (e != hipSuccess) return e;
  h->place_state.pbytes = pbytes;
  placement_leg(h, pbytes);
  if (h->v) return hipSuccess;
  e = alloc(h->v_block, pbytes);                                       // no candidate at all (no memory to search in): plain allocation
  h->v = h->v_block;
  return e;
}

// A reset replaces the particles: while the search has only ended for lack of time, and nobody outside has been given the arrays'
// addresses, it may run another leg and move v for nothing.
void resume_placement(pic_handle* h) {
  PlacementState& ps = h->place_state;
  if (!h->v_separate || ps.pbytes == 0 || ps.ptrs_exposed || ps.legs >= kMaxLegs || h->place.outcome != PIC_PLACED_TIMEOUT) return;
  (void)hipStreamSynchronize(h->stream);
  placement_leg(h, ps.pbytes);
}
