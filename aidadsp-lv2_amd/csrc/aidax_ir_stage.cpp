// aidax_ir_stage.cpp — the device half of the cabinet IR stage (aidax_ir_stage.h): the history, the IR and plan uploads and the
// launches of aidax_ir_mfma.hip behind every pass. Host logic only.
#include <algorithm>
#include <memory>

#include "aidax_ir_stage.h"
#include "aidax_snapshot_ring.h"

namespace aidax {

// Per stream a ring of the last R >= capacity + max_frames dry samples (aidax_kernels.h: IrArgs), fed by every pass (k_ir_append), and
// the K split's partial sums (aidax_ir_mfma.hip). With it, the device copy of the plan (IrPlan's layout) and the pinned snapshots it
// is uploaded from, stream-ordered with the passes (aidax_snapshot_ring.h).
struct IrHistory {
    DevBuf<float> ring;
    DevBuf<float> part;
    uint32_t ring_row = 0, mask = 0, split_cap = 1;
    DevBuf<uint8_t> d_plan;
    SnapshotRing plan_ring;              // (audio side)
    DevBuf<float> side;                  // the IR fade's side buffer, [n_streams][max_frames]: what the fade-out section of a fade pass convolves into
};

IrStage::~IrStage()
{
    for (IrSlot* bank : { plan.live, plan.parked })         // (the fragments in force and parked: IrSlot is a record of the plan's)
        for (int k = 0; k < IrPlan::kKeys; ++k) DevBuf<uint32_t>::adopt(bank[k].d_frag);
    delete pub_.exchange(nullptr);
}

void IrStage::prepare(const float* taps, uint32_t n_taps, IrSlot& ir)
{
    if (!has_history()) {
        auto h = std::make_unique<IrHistory>();
        const uint32_t R = pow2_at_least(capacity.load(std::memory_order_relaxed) + max_frames_);
        h->mask = R - 1;
        h->ring_row = R + kIrMirror;
        const size_t block = static_cast<size_t>(plan.n_streams) * max_frames_;
        const size_t budget = size_t(16) << 20;              // floats of partial sums (64 MiB)
        h->split_cap = static_cast<uint32_t>(std::max<size_t>(1, std::min<size_t>(64, budget / block)));
        const size_t ring_floats = plan.n_streams * static_cast<size_t>(h->ring_row);
        h->ring.alloc(ring_floats);
        if (h->split_cap > 1) h->part.alloc(block * h->split_cap);
        h->side.alloc(block);
        const size_t plan_bytes = plan.total_bytes();        // every section, whether a fade length is set or a stream blended or not
        h->d_plan.alloc(plan_bytes);
        h->plan_ring.alloc(plan_bytes);
        HIP_TRY(hipMemsetAsync(h->ring.get(), 0, sizeof(float) * ring_floats, wq_));
        HIP_TRY(hipStreamSynchronize(wq_));
        pub_.store(h.release(), std::memory_order_release);
    }
    if (taps) {
        const std::vector<uint32_t> frag = pack_ir_fragments(taps, n_taps, &ir.n_diag);
        ir.n_taps = n_taps;
        DevBuf<uint32_t> d;
        d.alloc(frag.size());
        ir.d_frag = d.release();                             // (the staged object's from here: staged_release)
        HIP_TRY(hipMemcpyAsync(ir.d_frag, frag.data(), frag.size() * sizeof(uint32_t), hipMemcpyHostToDevice, wq_));
        HIP_TRY(hipStreamSynchronize(wq_));                 // `frag` is pageable; the audio side must find the IR complete
    }
}

void IrStage::commit(int32_t slot, IrSlot& staged, hipEvent_t fence, hipStream_t q)
{
    HIP_TRY(hipEventRecord(fence, q));                       // the retired fragments are free once the passes before this point have run
    plan.commit(1 + slot, staged);
    (void)adopt();
}

// the passes already issued keep the plan they were issued with: the device copy is overwritten behind them, from a pinned snapshot
// that no later rebuild touches while it is in flight
void IrStage::flush_plan(hipStream_t s, bool any_pass)
{
    plan.rebuild(any_pass);
    const size_t bytes = plan.serialise(hist_->plan_ring.take());
    hist_->plan_ring.send(hist_->d_plan.get(), 0, bytes, s);
}

// k_ir_conv's arguments for one section of the plan, which lies at these offsets of the device copy
IrArgs IrStage::conv_args(const IrSection& sec, size_t items_off, size_t streams_off, float* out, uint32_t n_active, uint32_t n_frames) const
{
    const IrHistory* h = hist_;
    IrArgs a{};
    a.items = reinterpret_cast<const IrItem*>(h->d_plan.get() + items_off);
    a.streams = reinterpret_cast<const uint32_t*>(h->d_plan.get() + streams_off);
    a.n_items = sec.n_items; a.n_listed = sec.n_listed;
    a.ring = h->ring.get(); a.out = out; a.part = h->part.get();
    a.ring_row = h->ring_row; a.mask = h->mask; a.pos = pos_;
    a.n_streams = n_active; a.n_frames = n_frames;
    return a;
}

void IrStage::issue(hipStream_t s, float* d_out, uint32_t n_active, uint32_t n_frames)
{
    IrHistory* h = hist_;
    // the block's dry samples into the history (also while no IR is live), then the convolution over the history, in place on d_out,
    // of the streams the plan holds (one launch whatever the number of IRs)
    HIP_TRY(launch_ir_append(h->ring.get(), h->ring_row, h->mask, pos_, d_out, n_active, n_frames, s));
    if (plan.main.n_items) {
        IrArgs ia = conv_args(plan.main, 0, plan.plan_items_bytes(), d_out, n_active, n_frames);
        if (plan.identity) {
            // the identity plan over the prefix only: the grid of a one-IR pool (entries at or beyond n_active are skipped anyway)
            ia.n_items = std::min(ia.n_items, (n_active + kIrItemStreams - 1) / kIrItemStreams);
            ia.n_listed = n_active;
        }
        ia.n_splits = ir_k_splits(ia.n_items, n_frames, plan.main.max_diag, cus_, h->split_cap);
        HIP_TRY(launch_ir_conv(ia, s));
    }
    if (plan.n_mix) {
        // an IR change since the last pass: the old IRs over the same history into the side buffer (the fade-out section: the
        // same kernel, K split and fixed-order reduce, `part` reused behind the main section's reduce), then the crossfade of the
        // first min(F, n_frames) frames in place on d_out
        if (plan.fade_out.n_items) {
            IrArgs fa = conv_args(plan.fade_out, plan.fade_items_off(), plan.fade_streams_off(), h->side.get(), n_active, n_frames);
            fa.n_splits = ir_k_splits(fa.n_items, n_frames, plan.fade_out.max_diag, cus_, h->split_cap);
            HIP_TRY(launch_ir_conv(fa, s));
        }
        IrFadeArgs fm{};
        fm.mix = reinterpret_cast<const uint32_t*>(h->d_plan.get() + plan.fade_mix_off());
        fm.side = h->side.get(); fm.ring = h->ring.get(); fm.out = d_out;
        fm.n_mix = plan.n_mix; fm.ring_row = h->ring_row; fm.mask = h->mask; fm.pos = pos_;
        fm.n_streams = n_active; fm.n_frames = n_frames;
        fm.lf = std::min(plan.fade, n_frames);
        HIP_TRY(launch_ir_fade(fm, s));
    }
    if (plan.n_blend) {
        // blended streams: their B sides over the same history into their rows of the side buffer (the blend section: the same kernel,
        // K split and fixed-order reduce, `part` reused behind the earlier reduces), then the mix over all frames in place on d_out, at
        // the ramp positions of the plan plus the frames issued since it was built
        if (plan.blend.n_items) {
            IrArgs ba = conv_args(plan.blend, plan.blend_items_off(), plan.blend_streams_off(), h->side.get(), n_active, n_frames);
            ba.n_splits = ir_k_splits(ba.n_items, n_frames, plan.blend.max_diag, cus_, h->split_cap);
            HIP_TRY(launch_ir_conv(ba, s));
        }
        IrBlendArgs bm{};
        bm.list = reinterpret_cast<const IrBlendEntry*>(h->d_plan.get() + plan.blend_list_off());
        bm.side = h->side.get(); bm.ring = h->ring.get(); bm.out = d_out;
        bm.n_blend = plan.n_blend; bm.ring_row = h->ring_row; bm.mask = h->mask; bm.pos = pos_;
        bm.n_streams = n_active; bm.n_frames = n_frames;
        bm.k_off = plan.since_build;
        HIP_TRY(launch_ir_mix(bm, s));
    }
    plan.pass_issued(n_active, n_frames);
    pos_ = (pos_ + n_frames) & h->mask;
}

void IrStage::clear_stream(uint32_t stream, hipStream_t q)
{
    if (!adopt()) return;
    HIP_TRY(hipMemsetAsync(hist_->ring.get() + static_cast<size_t>(stream) * hist_->ring_row, 0, sizeof(float) * hist_->ring_row, q));
}

void IrStage::clear_all(hipStream_t q)
{
    (void)hipMemsetAsync(hist_->ring.get(), 0, sizeof(float) * plan.n_streams * static_cast<size_t>(hist_->ring_row), q);
}

}  // namespace aidax
