// elf_image_is_whole (csrc/elf_extent.hpp), the check a cached code object passes before it goes to the module loader: the files
// named on the command line (a code object hiprtc returned for gfx950, this program's own executable) are accepted whole, refused
// at EVERY shorter length (the cut the cache test makes, a third, included), refused with a section offset or a segment size
// pointing past the end, with a section-header table past the end, and with a foreign magic.  Exit status 0 = all as expected.
#include "elf_extent.hpp"
#include <cstdio>
#include <vector>
using namespace bf;

static int one(const char* path) {
  std::vector<char> c;
  if (FILE* f = std::fopen(path, "rb")) {
    c.resize(1 << 26);
    c.resize(std::fread(c.data(), 1, c.size(), f));
    std::fclose(f);
  }
  if (c.size() < sizeof(Elf64_Ehdr)) { std::printf("%s: cannot read\n", path); return 1; }
  int bad = !elf_image_is_whole(c.data(), c.size());
  const size_t n = c.size(), stride = n > 100000 ? 257 : 1;
  for (size_t k = 0; k < n; k += stride) {
    std::vector<char> t(c.begin(), c.begin() + k);     // (its own allocation: a read past the end is the sanitizer's to see)
    bad += elf_image_is_whole(t.data(), t.size());
  }
  { std::vector<char> t(c.begin(), c.begin() + n / 3); bad += elf_image_is_whole(t.data(), t.size()); }
  Elf64_Ehdr eh;
  std::memcpy(&eh, c.data(), sizeof(eh));
  {  // the last section that has bytes in the file: its offset moved past the end
    std::vector<char> t(c);
    for (int i = eh.e_shnum - 1; i >= 0; --i) {
      Elf64_Shdr sh;
      std::memcpy(&sh, t.data() + eh.e_shoff + (size_t)i * sizeof(sh), sizeof(sh));
      if (sh.sh_type == SHT_NOBITS || sh.sh_size == 0) continue;
      sh.sh_offset = n - sh.sh_size + 1;
      std::memcpy(t.data() + eh.e_shoff + (size_t)i * sizeof(sh), &sh, sizeof(sh));
      break;
    }
    bad += elf_image_is_whole(t.data(), t.size());
  }
  if (eh.e_phnum) {  // a segment larger than the file
    std::vector<char> t(c);
    Elf64_Phdr ph;
    std::memcpy(&ph, t.data() + eh.e_phoff, sizeof(ph));
    ph.p_filesz = n + 1;
    std::memcpy(t.data() + eh.e_phoff, &ph, sizeof(ph));
    bad += elf_image_is_whole(t.data(), t.size());
  }
  {  // the section-header table past the end, and a huge count whose product would wrap
    std::vector<char> t(c);
    Elf64_Ehdr e2 = eh;
    e2.e_shoff = n - 8;
    std::memcpy(t.data(), &e2, sizeof(e2));
    bad += elf_image_is_whole(t.data(), t.size());
    e2 = eh;
    e2.e_shoff = ~0ull - 16;
    std::memcpy(t.data(), &e2, sizeof(e2));
    bad += elf_image_is_whole(t.data(), t.size());
  }
  { std::vector<char> t(c); t[1] = 'F'; bad += elf_image_is_whole(t.data(), t.size()); }
  std::printf("%s: %zu bytes, unexpected answers %d\n", path, n, bad);
  return bad;
}

int main(int argc, char** argv) {
  int bad = 0;
  for (int i = 1; i < argc; ++i) bad += one(argv[i]);
  bad += one(argv[0]);
  std::printf("total unexpected: %d\n", bad);
  return bad != 0;
}
