// Host side of the work tables (work_tables.h): the geometry of the current device and the one cache of uploaded tables. One instance
// of each per process: the functions are inline, so the translation units that include this share their statics. No locking, as
// everywhere in the library's host code.
#pragma once
#include "common.h"
#include <array>
#include <map>
#include <tuple>

static inline int psam_current_device() { int dev = 0; (void)hipGetDevice(&dev); return dev; }

// CU / XCD counts, read once per DEVICE from the runtime (a full MI355X reports 256 CUs in 8 XCDs; a CPX / NPS partition fewer): one
// process may drive several GPUs
struct PsamDevGeom { int cus = 0, xcds = 0; };
inline const PsamDevGeom& psam_device_geometry() {
  static PsamDevGeom geom[64];
  const int dev = psam_current_device();
  PsamDevGeom& g = geom[dev & 63];
  if (g.cus > 0) return g;
  int v = 0;
  g.cus = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256;
  g.xcds = (hipDeviceGetAttribute(&v, hipDeviceAttributeNumberOfXccs, dev) == hipSuccess && v > 0) ? v : 8;
  (void)hipGetLastError();
  return g;
}

// kind of table = its builder in work_tables.h; the arguments are the builder's, in its order
enum { PSAM_TAB_GEMM = 0, PSAM_TAB_SPLITK, PSAM_TAB_GATTN, PSAM_TAB_WATTN_WORK, PSAM_TAB_WATTN_GEOM };
typedef std::array<long long, 5> PsamTableArgs;
inline WorkTable psam_build_table(int kind, const PsamTableArgs& a) {
  switch (kind) {
    case PSAM_TAB_GEMM: return gemm_work_table((int)a[0], (int)a[1], (int)a[2], (int)a[3]);
    case PSAM_TAB_SPLITK: return splitk_work_table((int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)a[4]);
    case PSAM_TAB_GATTN: return gattn_work_table((int)a[0], (int)a[1], (int)a[2]);
    case PSAM_TAB_WATTN_WORK: return wattn_work_list((int)a[0], (int)a[1], (int)a[2]);
    case PSAM_TAB_WATTN_GEOM: return wattn_geometry_table(a[0]);
  }
  return {};
}

// The table of (kind, args) on the current device, built and uploaded on first use (synchronously: the first call of a shape must run
// outside stream capture). A published table is never freed or rewritten: launches already enqueued and captured graphs keep its
// address. Null where the builder refuses the shape or the upload fails - then nothing is cached, and a retry builds again.
struct PsamDeviceTable { void* dev = nullptr; int grid = 0, rows = 0; };
inline const PsamDeviceTable* psam_device_table(int kind, const PsamTableArgs& args) {
  static std::map<std::tuple<int, int, PsamTableArgs>, PsamDeviceTable> tabs;   // kind, device, the builder's arguments
  const auto key = std::make_tuple(kind, psam_current_device(), args);
  auto it = tabs.find(key);
  if (it != tabs.end()) return &it->second;
  const WorkTable h = psam_build_table(kind, args);
  if (h.words.empty()) return nullptr;
  PsamDeviceTable t;
  t.grid = h.grid;
  t.rows = h.rows;
  const size_t bytes = h.words.size() * sizeof(int);
  if (hipMalloc(&t.dev, bytes) != hipSuccess || hipMemcpy(t.dev, h.words.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
    if (t.dev) (void)hipFree(t.dev);
    (void)hipGetLastError();
    return nullptr;
  }
  return &(tabs[key] = t);
}
