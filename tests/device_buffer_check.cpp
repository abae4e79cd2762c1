// Holds the owners of mcbrat3d_amd/csrc/mcbrat_devmem.h to their rules without a GPU: the four seam functions are defined here
// over malloc and free, each pair with a count of live blocks, of allocations and of frees, and a switch that fails the k-th
// allocation from now.  One line per scenario; every figure is the change the scenario itself made.
// Built and read by tests/test_device_buffer_host.py, once plainly and once with the sanitizers (the leak checker included).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "../mcbrat3d_amd/csrc/mcbrat_devmem.h"

namespace {

struct Heap {
  long long live = 0, allocs = 0, frees = 0, calls = 0, failAt = 0;
  size_t lastBytes = 0;
  void fail_kth(long long k) { failAt = calls + k; }
};
Heap gDevice, gPinned;

int heap_alloc(Heap &h, void **ptr, size_t bytes) {
  *ptr = nullptr;
  if (++h.calls == h.failAt) return 2;  // (hipErrorOutOfMemory)
  *ptr = malloc(bytes);
  if (!*ptr) return 2;
  ++h.live; ++h.allocs;
  h.lastBytes = bytes;
  return 0;
}
void heap_free(Heap &h, void *ptr) {
  free(ptr);
  --h.live; ++h.frees;
}

}  // namespace

namespace mcbrat {
int device_alloc(void **ptr, size_t bytes) { return heap_alloc(gDevice, ptr, bytes); }
void device_free(void *ptr) { heap_free(gDevice, ptr); }
int pinned_alloc(void **ptr, size_t bytes) { return heap_alloc(gPinned, ptr, bytes); }
void pinned_free(void *ptr) { heap_free(gPinned, ptr); }
}  // namespace mcbrat

namespace {

// what a scenario did to its heap since `from`
void line(const char *who, const char *scenario, const Heap &h, const Heap &from, const char *rest) {
  printf("%s %s: %s allocs=%lld frees=%lld live=%lld\n", who, scenario, rest, h.allocs - from.allocs, h.frees - from.frees, h.live - from.live);
}

// three buffers, left by early return when an allocation fails: the shape of mcbrat_trace_fates
template <typename B>
int three_buffers() {
  B a, b, c;
  if (int status = a.allocate(16)) return status;
  if (int status = b.allocate(5)) return status;
  if (int status = c.allocate(7)) return status;
  return 0;
}

template <typename B>
void scenarios(const char *who, Heap &h) {
  char rest[256];
  {
    const Heap from = h;
    B b;
    const int s1 = b.allocate(8), s2 = b.allocate(8);
    snprintf(rest, sizeof(rest), "status=%d,%d full=%d capacity=%zu", s1, s2, (int)(bool)b, b.capacity());
    line(who, "allocate twice, same size", h, from, rest);
  }
  {
    const Heap from = h;
    B b;
    const size_t n = 0;
    const int s = b.allocate(std::max<size_t>(n, 1));  // (as upload() asks)
    snprintf(rest, sizeof(rest), "status=%d nonnull=%d capacity=%zu", s, (int)(b.get() != nullptr), b.capacity());
    line(who, "allocate for no elements", h, from, rest);
  }
  {
    B b;
    (void)b.allocate(8);
    const Heap from = h;
    const auto *p = b.get();
    const int s1 = b.reserve(4);
    const bool kept1 = b.get() == p && b.capacity() == 8;
    const int s2 = b.reserve(8);
    const bool kept2 = b.get() == p && b.capacity() == 8;
    const Heap mid = h;
    const int s3 = b.reserve(9);
    snprintf(rest, sizeof(rest), "status=%d,%d,%d smaller kept=%d equal kept=%d (allocs=%lld frees=%lld) larger capacity=%zu bytes=%zu", s1, s2, s3, (int)kept1,
             (int)kept2, mid.allocs - from.allocs, mid.frees - from.frees, b.capacity(), h.lastBytes);
    line(who, "reserve", h, from, rest);
  }
  for (int full = 0; full < 2; ++full)
    for (int viaReserve = 0; viaReserve < 2; ++viaReserve) {
      B b;
      if (full) (void)b.allocate(8);
      const Heap from = h;
      h.fail_kth(1);
      const int s = viaReserve ? b.reserve(9) : b.allocate(8);
      snprintf(rest, sizeof(rest), "status=%d full=%d null=%d capacity=%zu", s, (int)(bool)b, (int)(b.get() == nullptr), b.capacity());
      line(who, full ? (viaReserve ? "failing reserve, full buffer" : "failing allocate, full buffer")
                     : (viaReserve ? "failing reserve, empty buffer" : "failing allocate, empty buffer"), h, from, rest);
    }
  {
    const Heap from = h;
    B a;
    (void)a.allocate(4);
    const auto *p = a.get();
    B b(std::move(a));
    snprintf(rest, sizeof(rest), "source empty=%d capacity=%zu target holds=%d capacity=%zu", (int)!a, a.capacity(), (int)(b.get() == p), b.capacity());
    line(who, "move construction", h, from, rest);
    const Heap mid = h;
    B c;
    (void)c.allocate(2);
    c = std::move(b);
    snprintf(rest, sizeof(rest), "source empty=%d capacity=%zu target holds=%d capacity=%zu", (int)!b, b.capacity(), (int)(c.get() == p), c.capacity());
    line(who, "move assignment over a full buffer", h, mid, rest);
    const Heap late = h;
    B &self = c;
    c = std::move(self);
    snprintf(rest, sizeof(rest), "holds=%d capacity=%zu", (int)(c.get() == p), c.capacity());
    line(who, "self-move", h, late, rest);
  }
  {
    const Heap from = h;
    h.fail_kth(2);
    const int s = three_buffers<B>();
    snprintf(rest, sizeof(rest), "status=%d", s);
    line(who, "three buffers, the second allocation fails", h, from, rest);
  }
  {
    const Heap from = h;
    B b;
    (void)b.allocate(3);
    b.reset();
    b.reset();
    snprintf(rest, sizeof(rest), "empty=%d capacity=%zu", (int)!b, b.capacity());
    line(who, "reset twice", h, from, rest);
  }
}

}  // namespace

int main() {
  scenarios<mcbrat::DeviceBuffer<double>>("device", gDevice);
  scenarios<mcbrat::PinnedBuffer<unsigned long long>>("pinned", gPinned);
  printf("end: device live=%lld allocs-frees=%lld pinned live=%lld allocs-frees=%lld\n", gDevice.live, gDevice.allocs - gDevice.frees, gPinned.live,
         gPinned.allocs - gPinned.frees);
  return gDevice.live == 0 && gPinned.live == 0 && gDevice.allocs == gDevice.frees && gPinned.allocs == gPinned.frees ? 0 : 1;
}
