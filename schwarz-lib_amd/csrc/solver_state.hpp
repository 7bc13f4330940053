// What the iterative local solvers (cg.hip, cg_f32.hip, chebyshev.hip, gmres.hip, bicgstab.hip) share on the host: the
// device-resident scalar state with its pinned mirror and the poll one step behind the launches, and the schedule of
// the chunks between two polls.  Part of schwz_internal.hpp, which includes it behind the owners it is built from
// ("Solver state").  Header-inline: nothing here is instantiated by the host-only translation units.
#pragma once

#include <climits>
#include <cstring>

namespace schwz {

// The scalar state of a solve in HBM (State: a plain struct whose `int stop_iter` is INT_MAX until the device has
// decided to stop), two pinned host slots and an event per slot.  The kernels advance the state; the host reads
// copies of it: poll() while a solve is being launched, read() behind it, read_blocking() at any later time.
// The device address is fixed from create() to destruction: recorded graphs and SpmvArgs::stop_iter hold it.
template <typename State>
class StateMirror {
public:
    // allocates everything and zeroes both sides (complete on return)
    int create()
    {
        int rc;
        if ((rc = d_.alloc(1, true)) || (rc = h_.alloc(2)) || (rc = ev_[0].create()) || (rc = ev_[1].create())) return rc;
        SCHWZ_HIP_TRY(hipDeviceSynchronize());
        return SCHWZ_OK;
    }
    State *dev() const { return d_; }
    // a pinned slot: slot 0 is where read() and read_blocking() leave their copy
    State &host(int slot) { return h_.p[slot]; }
    // start of a solve: no copy is in flight
    void begin()
    {
        pending_ = -1;
        bank_ = 0;
    }
    // between two solves (schwz_ras_restart): the device state back to what create() left, zeros, behind everything
    // enqueued on `st`; no copy is in flight
    int reset(hipStream_t st)
    {
        SCHWZ_HIP_TRY(hipMemsetAsync(d_, 0, sizeof(State), st));
        begin();
        return SCHWZ_OK;
    }
    // One step behind the launches: waits for the copy the last poll() enqueued and sets *stopped if the device had
    // decided by then; enqueues the next copy and its event on `st`.  The queue behind the launches never drains.
    int poll(hipStream_t st, bool *stopped)
    {
        if (pending_ >= 0) {
            SCHWZ_HIP_TRY(hipEventSynchronize(ev_[pending_]));
            if (h_.p[pending_].stop_iter != INT_MAX) *stopped = true;
        }
        SCHWZ_HIP_TRY(hipMemcpyAsync(&h_.p[bank_], d_, sizeof(State), hipMemcpyDeviceToHost, st));
        SCHWZ_HIP_TRY(hipEventRecord(ev_[bank_], st));
        pending_ = bank_;
        bank_ ^= 1;
        return SCHWZ_OK;
    }
    // the state behind everything enqueued on `st` so far, to host(0) (synchronises st)
    int read(hipStream_t st)
    {
        SCHWZ_HIP_TRY(hipMemcpyAsync(&h_.p[0], d_, sizeof(State), hipMemcpyDeviceToHost, st));
        SCHWZ_HIP_TRY(hipStreamSynchronize(st));
        return SCHWZ_OK;
    }
    // ... behind everything enqueued on any stream (synchronises the device)
    int read_blocking()
    {
        SCHWZ_HIP_TRY(hipDeviceSynchronize());
        SCHWZ_HIP_TRY(hipMemcpy(&h_.p[0], d_, sizeof(State), hipMemcpyDeviceToHost));
        return SCHWZ_OK;
    }

private:
    Dev<State> d_;
    Pinned<State> h_;
    Event ev_[2];
    int pending_ = -1, bank_ = 0;
};

// Iterations between two polls of a tolerance solve: 16, then 32, then 64 from there on -- a stop is seen early
// while a solve is short, and a long one is not held up by its polls (CG, fp32 CG, Chebyshev; GMRES polls per restart
// cycle, BiCGSTAB per SCHWZ_BICGSTAB_POLL_BATCH iterations).
struct ChunkSchedule {
    static constexpr int kChunks[3] = {16, 32, 64};
    int step = 0;
    // end of the chunk that starts at iteration `it`; without a poll, or where the next poll would fall on the end
    // of the solve, everything up to max_iters
    int end(int it, int max_iters, bool poll) const
    {
        return poll && it + kChunks[step] < max_iters ? it + kChunks[step] : max_iters;
    }
    void grow()
    {
        if (step < 2) ++step;
    }
};

}  // namespace schwz
