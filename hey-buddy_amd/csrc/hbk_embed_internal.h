// What the speech-embedding translation units share on the host. hbk_embed.hip: the plan
// realised on the device, the launcher and the hbk_embed_* entry points; hbk_embed_exact.hip: the
// exact-f32 chain kernel; hbk_embed_x3.hip: the generic split-f16 chain kernel and its phase
// counters; hbk_embed_band.hip: the banded pattern kernels p0 and p1; hbk_embed_stream.hip: the
// streaming pattern kernels p0s, p1s, p2s and t3s. The host reaches a chain kernel only through
// its address (hipLaunchKernel), so one function per family crosses a unit and no kernel symbol
// does (addr is the cast those functions share). Device helpers that several families use are in
// hbk_embed_dev.h, the argument structs in hbk_embed_args.h, the planner in hbk_embed_plan.h.
#pragma once

namespace hbk {

// The kernel of its family that a KernelChoice (hbk_embed_plan.h) names: kernel_address in
// hbk_embed.hip picks the family. The choice travels as its fields (kind = int(Kern)): the
// planner's types are in an unnamed namespace, so a function over them cannot cross a unit.
const void* embed_exact_kernel(int n, bool flag);             // Kern::exact
const void* embed_x3_kernel(int n, bool flag);                // Kern::x3
const void* embed_band_kernel(int kind, int n, bool flag);    // Kern::p0_band, Kern::p1
const void* embed_stream_kernel(int kind, bool flag);         // Kern::p0s, Kern::p1s, Kern::p2s, Kern::t3s

namespace {
template <class A>
const void* addr(void (*kernel)(A)) {
  return reinterpret_cast<const void*>(kernel);
}
}  // namespace

}  // namespace hbk
