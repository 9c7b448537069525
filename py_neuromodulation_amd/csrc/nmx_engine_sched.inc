// nmx_engine_sched.inc -- the schedule of a chunk and of a batch: which stream a launch goes to, which events say a chunk
// is complete, when a host input buffer may be overwritten.  Included by nmx_engine.inc; the plan owns one Schedule.
// The whole dependency structure is in this file; run_chunk and process_batch_impl (nmx_engine_run.inc) and the stages'
// launchers call its operations and name no event.  tests/chunk_schedule_cases.py pins it.
//
// A chunk (nw hops) of parity `par` = chunk_seq & 1:
//
//   main    begin_chunk ..front, pre-processing.. bank --+-- [Hilbert] --+-- time/osc, coherence, [sharp waves] -- end_main
//   bursts                        fork_bursts (mode 1) --+- or (2, 4) ---+-> [Hilbert] walk, statistics -- join_bursts
//   sharp                         fork_sharp (mode 4) ---+-> sharp waves -- join_sharp
//   finalize   (normaliser / projection attached)  begin_finalize: behind all of the above .. end_finalize
//
// The tensors the side streams read (envelopes, thresholds, sharp-wave series and flags) exist twice: a chunk's main stream
// does not wait for the previous chunk's side streams -- its re-reference, notch and FIR bank run under them -- only for
// the chunk before that, whose set it is about to overwrite (begin_chunk).
//
// A batch from host memory adds the copy streams: chunk k's samples go to input buffer k & 1 on the copy-in stream
// (wait_input_free .. input_copied), its rows come back on the copy-out stream behind wait_done.

// NMX_OVERLAP: what runs beside the main stream's throughput kernels (3 and anything above 4: as 2)
enum class Overlap {
  ONE_STREAM = 0,        // nothing
  HILBERT_WALK = 1,      // Hilbert + threshold walk + run statistics on the bursts side stream
  WALK = 2,              // threshold walk + run statistics
  WALK_SHARP = 4,        // ... and the sharp-wave analysis on a second side stream (the default)
};
static Overlap overlap_mode(int v) { return v == 0 || v == 1 || v == 4 ? (Overlap)v : Overlap::WALK; }

// How one batch runs: on the plan's streams behind main stream `s` (the plan's, or the caller's), or -- `inline_all`, the
// one-window call of a real-time loop and any host batch of a few hops -- everything on `s`: no side, finalize or copy
// streams.  A value of the batch; the plan's mode is never changed.
struct BatchSched {
  be_stream_t s;
  bool inline_all;
};

struct Schedule {
  be_stream_t main = nullptr;          // the plan's own stream
  be_stream_t side_bursts = nullptr;   // high priority: the sequential, latency-bound part of the bursts chain
  be_stream_t side_sharp = nullptr;    // the sharp-wave analysis next to Hilbert + time / oscillatory
  be_stream_t finalize = nullptr;      // feature normaliser + "rows ready" of a chunk, behind its main and side streams
  be_stream_t copy_in = nullptr;       // host buffers move chunk by chunk next to the kernels
  be_stream_t copy_out = nullptr;      // the features' way back: its waits for a chunk's completion do not hold the next input copy
  be_stream_t last_stream = nullptr;   // main stream of the last batch (may be the caller's): state calls wait for it
  be_event_t ev_fork{}, ev_fork_d{};   // main -> bursts / sharp side stream
  be_event_t ev_join[2]{}, ev_join_d[2]{};   // end of the chunk's work there, per parity
  be_event_t ev_main[2]{};             // end of the chunk's main stream
  be_event_t ev_done[2]{};             // end of its finalize step
  be_event_t ev_in_free[2]{};          // the samples of the chunk that used input buffer i have been consumed (re-referenced / filtered)
  bool in_free[2] = {false, false};    // ... was recorded for that chunk (else: the chunk's completion)
  be_event_t ev_h2d{};                 // a chunk's samples have arrived
  long long chunk_seq = 0;             // chunks launched so far: parity selects the double-buffered hand-off tensors
  Overlap mode = Overlap::WALK_SHARP;
  bool bursts = false, sharp = false;  // the plan has those stages (nmx_plan_create, behind the stages' build)

  // the only lists of streams (f(stream, high priority)) and events: create and destroy walk them
  template <class F>
  void each_stream(F f) {
    f(main, false); f(side_bursts, true); f(finalize, false); f(side_sharp, false); f(copy_in, false); f(copy_out, false);
  }
  template <class F>
  void each_event(F f) {
    f(ev_fork); f(ev_fork_d); f(ev_h2d);
    for (int i = 0; i < 2; ++i) { f(ev_join[i]); f(ev_join_d[i]); f(ev_main[i]); f(ev_in_free[i]); f(ev_done[i]); }
  }
  // Nothing of the plan's is in flight any more: what destroy, state reset, export and import wait for.  (The copy streams
  // are drained by the batch that used them.)
  void quiesce() {
    be_sync(main);
    if (last_stream && last_stream != main) be_sync(last_stream);   // batch launched on a caller's stream
    be_sync(side_bursts);
    be_sync(side_sharp);
    be_sync(finalize);
  }

  int parity() const { return (int)(chunk_seq & 1); }
  // ---- the mode of a batch: each predicate includes "the plan has that stage"
  bool hilbert_on_side(const BatchSched& b) const { return bursts && !b.inline_all && mode == Overlap::HILBERT_WALK; }
  bool walk_on_side(const BatchSched& b) const { return bursts && !b.inline_all && (mode == Overlap::WALK || mode == Overlap::WALK_SHARP); }
  bool bursts_on_side(const BatchSched& b) const { return hilbert_on_side(b) || walk_on_side(b); }
  bool sharp_on_side(const BatchSched& b) const { return sharp && !b.inline_all && mode == Overlap::WALK_SHARP; }
  be_stream_t in_stream(const BatchSched& b) const { return b.inline_all ? b.s : copy_in; }
  be_stream_t out_stream(const BatchSched& b) const { return b.inline_all ? b.s : copy_out; }

  // ---- one chunk
  // The chunk of parity parity() begins on b.s: it overwrites the side tensors of the chunk two back (whatever the mode of the
  // batch that launched that one).
  void begin_chunk(const BatchSched& b) {
    const int par = parity();
    if (chunk_seq >= 2) {
      be_stream_wait(b.s, ev_join[par]);
      be_stream_wait(b.s, ev_join_d[par]);
    }
    // (with the Hilbert kernel on the side stream the previous chunk's may still read the band series `yb`, which exists once)
    if (hilbert_on_side(b) && chunk_seq >= 1) be_stream_wait(b.s, ev_join[par ^ 1]);
  }
  // -> the bursts side stream, behind everything on b.s so far
  be_stream_t fork_bursts(const BatchSched& b) {
    be_event_record(ev_fork, b.s);
    be_stream_wait(side_bursts, ev_fork);
    return side_bursts;
  }
  // the bursts chain of this chunk ends here on `sb`, the stream it ran on
  void join_bursts(const BatchSched& b, be_stream_t sb) {
    if (bursts_on_side(b)) be_event_record(ev_join[parity()], sb);
  }
  be_stream_t fork_sharp(const BatchSched& b) {
    be_event_record(ev_fork_d, b.s);
    be_stream_wait(side_sharp, ev_fork_d);
    return side_sharp;
  }
  void join_sharp() { be_event_record(ev_join_d[parity()], side_sharp); }
  // (no join on the main stream: the chunk is finished by whoever waits for its events)
  void end_main(const BatchSched& b) { be_event_record(ev_main[parity()], b.s); }
  // the events that complete the kernels of the chunk of parity `par`, launched by batch `b`
  template <class F>
  void each_kernel_event(const BatchSched& b, int par, F f) {
    f(ev_main[par], true);   // (true: recorded on the chunk's own main stream)
    if (bursts_on_side(b)) f(ev_join[par], false);
    if (sharp_on_side(b)) f(ev_join_d[par], false);
  }
  // The finalize step of this chunk (normaliser, projection) -> its stream: the finalize stream behind the chunk's kernels,
  // or the batch's one stream.  end_finalize marks the rows complete, and the chunk over.
  be_stream_t begin_finalize(const BatchSched& b) {
    if (b.inline_all) return b.s;
    each_kernel_event(b, parity(), [&](be_event_t& e, bool) { be_stream_wait(finalize, e); });
    return finalize;
  }
  void end_finalize(be_stream_t sf) { be_event_record(ev_done[parity()], sf); }
  void next_chunk() { ++chunk_seq; }
  // Stream `st` waits until the chunk of parity `par` is complete (its rows final).  `finalized`: it had a finalize step;
  // `own_main`: st IS the chunk's main stream.
  void wait_done(const BatchSched& b, be_stream_t st, int par, bool finalized, bool own_main) {
    if (finalized) { be_stream_wait(st, ev_done[par]); return; }
    each_kernel_event(b, par, [&](be_event_t& e, bool on_main) { if (!(on_main && own_main)) be_stream_wait(st, e); });
  }

  // ---- the two input buffers of a host batch (chunk k uses buffer k & 1)
  // before chunk k's samples are copied: the chunk two back read this buffer -- its samples consumed (its pre-processing
  // done), or, in a plan whose features read the samples themselves, the chunk complete (same parity as the chunk about to
  // start; its events not yet re-recorded)
  void wait_input_free(const BatchSched& b, int k, bool finalized) {
    if (k < 2) return;
    if (in_free[k & 1]) be_stream_wait(in_stream(b), ev_in_free[k & 1]);
    else wait_done(b, in_stream(b), parity(), finalized, false);
  }
  // the chunk's samples are on their way: the main stream starts behind them
  void input_copied(const BatchSched& b) {
    if (b.inline_all) return;
    be_event_record(ev_h2d, in_stream(b));
    be_stream_wait(b.s, ev_h2d);
  }
  // What run_chunk records once nothing more reads chunk k's samples (null: the batch does not recycle its buffers that
  // way), and whether it did.
  be_event_t* input_consumed_event(const BatchSched& b, int k) { return b.inline_all ? nullptr : &ev_in_free[k & 1]; }
  void input_consumed(int k, bool recorded) { in_free[k & 1] = recorded; }
  // an error in mid-batch: nothing returns to the caller before the batch's streams have drained
  void drain(const BatchSched& b) {
    be_sync_quiet(in_stream(b));
    be_sync_quiet(out_stream(b));
    be_sync_quiet(b.s);
  }
};
