/* cli.c -- the ways out of the program that name the GPU library or the version (cli.h) */
#include "cli.h"
#include "sigtk_gpu.h"
#include "version.h"

void gpu_fail(const char *tool, const char *what, int rc) {
    if (!tool) {
        ERROR(what, "%s %s", sgk_strerror(rc), sgk_last_hip_error());
        die_now();
    }
    ERROR(tool, "%s failed: %s %s", what, sgk_strerror(rc), sgk_last_hip_error());
    die_flushed();
}

void die_read_error(int code) {
    fprintf(stderr, "Error in slow5_get_next. Error code %d\n", code);
    die_now();
}

void version_exit(void) {
    fprintf(stdout, "sigtk %s\n", SIGTK_VERSION);
    exit(EXIT_SUCCESS);
}
