// elf_extent: whether a code object read from the on-disk cache (jit_cache.hip) is a WHOLE ELF64 image.
// hipModuleLoadData takes a pointer and no length: it trusts the image's own headers for its extents, and on a truncated file it
// reads past the buffer (observed: std::bad_alloc thrown inside the runtime, which ends the process).  So a cached file goes to
// the loader only if every table, section and segment its ELF headers name lies inside the bytes that were read; anything else
// is "a file that does not load" and is rebuilt.  (hiprtc returns a plain ELF64 code object for the one target it is given.)
// Plain C++, no HIP: tests/c/elf_extent_check.cpp builds it for the host.
#pragma once
#include <elf.h>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace bf {

inline bool elf_image_is_whole(const char* data, size_t size) {
  Elf64_Ehdr eh;
  if (size < sizeof(eh)) return false;
  std::memcpy(&eh, data, sizeof(eh));
  if (std::memcmp(eh.e_ident, ELFMAG, SELFMAG) != 0 || eh.e_ident[EI_CLASS] != ELFCLASS64) return false;
  auto inside = [&](uint64_t off, uint64_t len) { return off <= size && len <= size - off; };
  if (eh.e_shnum == 0 || eh.e_shentsize != sizeof(Elf64_Shdr) || !inside(eh.e_shoff, (uint64_t)eh.e_shnum * sizeof(Elf64_Shdr))) return false;
  if (eh.e_phnum != 0 && (eh.e_phentsize != sizeof(Elf64_Phdr) || !inside(eh.e_phoff, (uint64_t)eh.e_phnum * sizeof(Elf64_Phdr)))) return false;
  for (unsigned i = 0; i < eh.e_shnum; ++i) {
    Elf64_Shdr sh;
    std::memcpy(&sh, data + eh.e_shoff + (uint64_t)i * sizeof(sh), sizeof(sh));
    if (sh.sh_type != SHT_NOBITS && !inside(sh.sh_offset, sh.sh_size)) return false;
  }
  for (unsigned i = 0; i < eh.e_phnum; ++i) {
    Elf64_Phdr ph;
    std::memcpy(&ph, data + eh.e_phoff + (uint64_t)i * sizeof(ph), sizeof(ph));
    if (!inside(ph.p_offset, ph.p_filesz)) return false;
  }
  return true;
}

}  // namespace bf
