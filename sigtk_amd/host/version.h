/* version.h -- the reference version whose CLI sigtk-amd mirrors (src/sigtk.h:11) */
#ifndef SIGTK_AMD_VERSION_H
#define SIGTK_AMD_VERSION_H
#define SIGTK_VERSION "0.2.0"
#endif
