// Stand-alone host program: the argument checks of the cell-list build (gelslim_depth_amd/csrc/gsd_cell_lists.h) need no device.
// Build for the host with -fsanitize=address,undefined and run; exit status 0 when every refusal has its code and names its
// entry point.  tests/test_cell_lists_host.py does both.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "gsd_cell_lists.h"

static char g_message[512];
void gsd_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_message, sizeof g_message, fmt, ap);
  va_end(ap);
}

static int failures = 0;
static void expect(const char* label, const GsdCellCall& Q, bool fill, int want) {
  g_message[0] = 0;
  const int got = gsd_cell_check(Q, fill);
  const bool named = want == GSD_OK ? g_message[0] == 0 : strncmp(g_message, Q.what, strlen(Q.what)) == 0 && g_message[strlen(Q.what)] == ':';
  if (got != want || !named) {
    printf("FAIL %s: code %d (want %d), message \"%s\"\n", label, got, want, g_message);
    ++failures;
  } else {
    printf("ok   %s: %d %s\n", label, got, g_message);
  }
}

int main() {
  const int64_t ncells = 4097;
  std::vector<int64_t> store((size_t)gsd_cell_words(ncells) / 2 + 2);      // 8-byte aligned
  int32_t* cells = reinterpret_cast<int32_t*>(store.data());
  std::vector<float> geometry(9);
  std::vector<int32_t> list(16);
  for (const char* what : {"gsd_mesh_depth_count", "gsd_mesh_depth_fill", "gsd_mesh_volume_count", "gsd_mesh_volume_fill"}) {
    const bool fill = strstr(what, "_fill") != nullptr;
    const GsdCellCall ok{what, geometry.data(), 1, 1 << 24, ncells, cells, gsd_cell_words(ncells), list.data(), (int64_t)list.size()};
    expect("accepted", ok, fill, GSD_OK);
    GsdCellCall q = ok;
    q.geometry = nullptr;
    expect("null geometry", q, fill, GSD_ERR_BAD_ARG);
    q = ok, q.cells = nullptr;
    expect("null cells", q, fill, GSD_ERR_BAD_ARG);
    q = ok, q.list = nullptr;
    expect("null list", q, fill, fill ? GSD_ERR_BAD_ARG : GSD_OK);
    q = ok, q.cells_elems = gsd_cell_words(ncells) - 1;
    expect("short workspace", q, fill, GSD_ERR_WORKSPACE);
    q = ok, q.cells_elems = 0;
    expect("empty workspace", q, fill, GSD_ERR_WORKSPACE);
    q = ok, q.cells = cells + 1;
    expect("misaligned cells", q, fill, GSD_ERR_BAD_ARG);
    q = ok, q.T = 0;
    expect("T = 0", q, fill, GSD_ERR_BAD_ARG);
    q = ok, q.T = (1 << 24) + 1;
    expect("T above the limit", q, fill, GSD_ERR_BAD_ARG);
    q = ok, q.T = -5;
    expect("T negative", q, fill, GSD_ERR_BAD_ARG);
    q = ok, q.list_elems = 0;
    expect("empty list", q, fill, fill ? GSD_ERR_BAD_ARG : GSD_OK);
    q = ok, q.list_elems = (int64_t)INT32_MAX + 1;
    expect("list above 2^31 - 1", q, fill, fill ? GSD_ERR_BAD_ARG : GSD_OK);
  }
  if (gsd_cell_words(1) != 5 || gsd_cell_words(int64_t(1) << 24) != 2 + 2 * (int64_t(1) << 24) + 1) {
    printf("FAIL gsd_cell_words\n");
    ++failures;
  }
  printf("%d failure(s)\n", failures);
  return failures != 0;
}
