// device_info.hpp — DeviceInfo: what a launcher is told about the device it launches on (filled by host.hpp's device_info()).
#pragma once

namespace clfa {

struct DeviceInfo {
  int device = 0;
  int num_cus = 256;
};

}  // namespace clfa
