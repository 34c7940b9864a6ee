// vp8g_argb_batch.h -- one batch of device-resident ARGB pictures on their way into slots of a tensor, those that are
// cropped / rescaled through the planar rescaler first (vp8g_scale_argb.hip).  A wrapper over the public
// makers and launches of include/vp8g.h, which holds what they leave to the caller: the running offsets and counters of
// a launch.  The pipeline's lossless sink and the animated call's planar route both build their batches here.
#pragma once

#include <vector>

#include "../host/vp8_front.h"
#include "vp8g_device.h"

namespace vp8g {

struct ArgbScaleBatch {
	std::vector<Vp8gScaleArgbDesc> scale;    // the rescaled pictures, in the order of add()
	std::vector<Vp8gTensorArgbDesc> tensor;  // every picture, in the order of add() / add_whole()

	// What one rescaled picture adds to a batch, in bytes: `work` in the work area (behind its head: head_bytes), `scaled`
	// among the scaled pictures, `descs` for its descriptor and its four plane descriptors in the head.  A caller prices
	// and lays out a batch from these before it builds it.  All zero + EINVAL for an option that does not fit the picture.
	struct Need {
		uint64_t work, scaled, descs;
	};
	static Need need(uint32_t width, uint32_t height, const Vp8gScaleOpt* opt) {
		Vp8fScaleGeom g;
		if (vp8f_scale_resolve_argb(width, height, opt, &g) != 0) return errno = EINVAL, Need{0, 0, 0};
		return Need{al256(vp8g_scale_argb_work_size(width, height, opt)), al256(4ull * g.out_w * g.out_h),
		            sizeof(Vp8gScaleArgbDesc) + 4u * sizeof(Vp8gScaleDesc)};
	}
	// The head of the work area of a batch with n rescaled pictures.
	static uint64_t head_bytes(uint32_t n) { return n ? vp8g_scale_argb_head_size(n) : 0u; }

	// An empty batch of n rescaled pictures (at most), whose scaled pictures lie from `scaled0` of the buffer on.
	void begin(uint32_t n, uint64_t scaled0) {
		scale.clear(), tensor.clear();
		work_ = head_bytes(n), scaled_ = scaled0;
		planes_ = t_split_ = t_scale_ = t_merge_ = t_tensor_ = 0;
	}
	// The width x height picture at `src` of the buffer, rescaled by `opt`, into the slot at `slot` of the tensor.
	// 0, or -1 + errno as vp8g_make_scale_argb_desc / vp8g_make_tensor_argb_desc (the batch is as before).
	int add(uint32_t width, uint32_t height, uint64_t src, const Vp8gScaleOpt* opt, const Vp8gTensorOpt* t, uint32_t channels, uint64_t slot) {
		Vp8gScaleArgbDesc s;
		if (vp8g_make_scale_argb_desc(width, height, src, opt, work_, scaled_, planes_, t_split_, t_scale_, t_merge_, &s) != 0 ||
		    add_whole(t, channels, scaled_, slot) != 0)
			return -1;
		scale.push_back(s);
		planes_ += s.nplanes, t_split_ += s.split_ntasks, t_scale_ += s.scale_ntasks, t_merge_ += s.merge_ntasks;
		work_ = al256(work_ + s.work_bytes), scaled_ = al256(scaled_ + 4ull * s.width * s.height);
		return 0;
	}
	// A picture of the tensor's size at `src` that goes as it is.
	int add_whole(const Vp8gTensorOpt* t, uint32_t channels, uint64_t src, uint64_t slot) {
		Vp8gTensorArgbDesc d;
		if (vp8g_make_tensor_argb_desc(t, channels, src, slot, t_tensor_, &d) != 0) return -1;
		tensor.push_back(d);
		t_tensor_ += d.ntasks;
		return 0;
	}
	// The rescaler over the pictures of add(), then the tensor kernel over every picture, on `stream`.  d_scale and
	// d_tensor: the device copies of the two arrays, which the caller has uploaded on the same stream; d_buf: what the
	// pictures' offsets count from, sources and scaled pictures alike; d_work: the work area.  Asynchronous; on a failure
	// errno is the entry point's.
	Status launch(const Vp8gScaleArgbDesc* d_scale, const Vp8gTensorArgbDesc* d_tensor, uint8_t* d_buf, uint8_t* d_work, const Vp8gTensorOpt* t,
	              uint32_t channels, void* d_out, hipStream_t stream) const {
		if (!scale.empty())
			if (int rc = vp8g_scale_argb_batch_device(scale.data(), d_scale, (uint32_t)scale.size(), d_buf, d_work, d_buf, stream); rc != 0)
				return capi_status(rc, "lossless scale launch");  // (the pipeline's text; the animated call passes errno on)
		return capi_status(vp8g_tensor_batch_device_argb(tensor.data(), d_tensor, (uint32_t)tensor.size(), t, channels, d_buf, d_out, stream),
		                   "tensor launch");
	}

   private:
	uint64_t work_ = 0, scaled_ = 0;  // where the next picture's planes / scaled picture go
	uint32_t planes_ = 0, t_split_ = 0, t_scale_ = 0, t_merge_ = 0, t_tensor_ = 0;  // the launches' running totals
};

}  // namespace vp8g
