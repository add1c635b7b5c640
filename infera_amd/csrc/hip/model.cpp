// model.cpp -- infera_load_model's device half: every scheduled step's constants uploaded to each selected GPU, once, and owned there by the
// DeviceModel (what each kernel family keeps in HBM and how it is packed: steps.cpp).  (engine.rs:49-55: the reference builds a Tract plan
// here; nothing model-dependent is left per chunk.)
#include "runtime.hpp"
#include "../host/onnx_model.hpp"

namespace infera_hip {
namespace rt {

void *upload_bytes(DeviceModel &dm, hipStream_t stream, const void *src, size_t bytes) {
  if (bytes == 0) return nullptr;
  dm.allocations.reserve(dm.allocations.size() + 1);  // (the push_back below cannot fail)
  void *d = nullptr;
  HIP_TRY(hipMalloc(&d, bytes));
  hipError_t e = hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) {
    (void)hipFree(d);
    hip_fail(e, "hipMemcpy(weights)");
  }
  dm.allocations.push_back(d);
  return d;
}

void upload_to_device(const LoadedModel &m, DeviceModel &dm) {
  UnsafeOpGuard guard;
  const Upload up{m, dm, ctx_for_slot(slot_of_ordinal(dm.device)).stream};  // also does hipSetDevice
  dm.steps.resize(m.plan.steps.size());
  for (size_t i = 0; i < dm.steps.size(); i++) upload_step(up, i);
}

}  // namespace rt
using namespace rt;

DeviceModel::~DeviceModel() {
  if (device < 0) return;
  UnsafeOpGuard guard;
  if (hipSetDevice(device) != hipSuccess) return;
  (void)hipDeviceSynchronize();
  for (void *p : allocations) (void)hipFree(p);
}

std::shared_ptr<LoadedModel> build_model(const std::string &name, const std::string &path, const std::string &output_select) {
  static std::atomic<uint64_t> next_uid{1};
  auto m = std::make_shared<LoadedModel>();
  m->uid = next_uid.fetch_add(1);
  m->name = name;
  onnx::Model om = onnx::parse_file(path);
  m->plan = lower_model(om, output_select);
  schedule(*m);
  const DeviceSet &ds = devices();
  if (ds.ids.empty()) {
    // No GPU: the model is registered (metadata, shape validation and the error paths above the
    // compute call keep working) but cannot execute; see run_host/run_device.
    m->device_error = ds.why;
    log_msg(1, "model '" + name + "' loaded without a GPU: " + ds.why + "; predictions will fail");
    return m;
  }
  for (size_t i = 0; i < ds.ids.size(); i++) {
    auto dm = std::make_unique<DeviceModel>();
    dm->device = ds.ids[i];
    dm->num_cus = ds.cus[i];
    upload_to_device(*m, *dm);
    m->dev.push_back(std::move(dm));
  }
  return m;
}

}  // namespace infera_hip
