// cl_dconv.h — drop-in for the reference's cl_dconv.h (cl_dconv.h:15-67).
#ifndef __CL_DCONV_H__
#define __CL_DCONV_H__
#include "cl_conv.h"

namespace cl_conv {

class Cldconv {
  int irsize, vsize;
  clfa_dconv *dc;
  void (*err)(std::string s, void *uData);
  void *userData;
  int cl_err;

  static void msg(std::string str, void *userData) {
    if (userData == NULL) std::cout << str << std::endl;
  }
  Cldconv(const Cldconv &);
  Cldconv &operator=(const Cldconv &);

 public:
  /** cvs - impulse response size; vsize - processing vector size */
  Cldconv(cl_device_id device_id, int cvs, int vsize, void (*errs)(std::string s, void *d) = NULL,
          void *uData = NULL);
  /** extension: `channels` independent instances in one object (arrays become channel-major) */
  Cldconv(cl_device_id device_id, int cvs, int vsize, int channels, void (*errs)(std::string s, void *d), void *uData);
  ~Cldconv();
  const char *cl_error_string(int err) { return cl_string(err); }
  int push_ir(float *ir);
  int convolution(float *output, float *input);
  int convolution(float *out, float *in1, float *in2);
  /** device-resident extension (in2 may be NULL; out must not be an input) */
  int convolution_device(void *out, const void *in1, const void *in2, void *stream = 0);
  /** device-resident push_ir: row c at c * channel_stride floats (clfa_dconv_push_ir_dev) */
  int push_ir_device(const void *ir, long channel_stride, void *stream = 0);
  /** nblocks consecutive blocks per channel, rows of nblocks * vsize floats (in2 may be NULL); blocking */
  int convolution_blocks(float *out, float *in1, float *in2, long nblocks);
  /** ... device-resident, row c at c * stride floats: the same as nblocks convolution_device calls
      (clfa_dconv_process_blocks_dev) */
  int convolution_blocks_device(void *out, long out_stride, const void *in1, const void *in2, long in_stride,
                                long nblocks, void *stream = 0);
  /** "k_dconvb_fir" (static form) or "loop" (two inputs) */
  const char *blocks_kernel_name(bool time_varying = false);
  int channels() { return clfa_dconv_channels(dc); }
  int wp() { return clfa_dconv_wp(dc); }
  int get_cl_err() { return cl_err; }
};
}  // namespace cl_conv
#endif
