// The status rule of the launch layer (csrc/nsid_common.h: nsid_note_launch / nsid_launch_status), host code only: the first error
// of an entry is the one reported, and reading clears it. Needs no device and touches none. tests/test_launch_layer_cpu.py builds
// and runs it: exit status 0 = every check held (else the number of the first one that did not); stdout names the error strings
// stderr must carry, in order, and after "not:" the one it must not.
#include "../neuralsampleid_amd/csrc/nsid_common.h"

int main() {
  int check = 0;
#define EXPECT(cond)                                           \
  do {                                                         \
    ++check;                                                   \
    if (!(cond)) {                                             \
      printf("check %d failed: %s\n", check, #cond);           \
      return check;                                            \
    }                                                          \
  } while (0)
  // nothing noted, and successes only
  EXPECT(nsid_launch_status() == NSID_OK);
  nsid_note_launch(hipSuccess);
  nsid_note_launch(hipSuccess);
  EXPECT(nsid_launch_status() == NSID_OK);
  // an error followed by two successes: reported once
  nsid_note_launch(hipErrorInvalidValue);
  nsid_note_launch(hipSuccess);
  nsid_note_launch(hipSuccess);
  EXPECT(nsid_launch_status() == NSID_ELAUNCH);
  EXPECT(nsid_launch_status() == NSID_OK);
  // two different errors: the first one is kept
  nsid_note_launch(hipErrorInvalidConfiguration);
  nsid_note_launch(hipErrorOutOfMemory);
  EXPECT(nsid_launch_status() == NSID_ELAUNCH);
  EXPECT(nsid_launch_status() == NSID_OK);
  printf("%s\n%s\nnot: %s\n", hipGetErrorString(hipErrorInvalidValue), hipGetErrorString(hipErrorInvalidConfiguration),
         hipGetErrorString(hipErrorOutOfMemory));
  return 0;
}
