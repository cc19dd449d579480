/* segopt_check.c -- the list parsers of jnn --segmenter, prefix --adaptor and prefix --polya (sigtk_amd/host/segopt.h)
 * over well-formed and malformed lists.  A stand-alone host program: build it with -fsanitize=address,undefined
 * (tests/test_segmenter_cli_cpu.py does) and run it; it exits 0 when every list is taken or refused as listed. */
#include <stdio.h>

#include "../sigtk_amd/host/segopt.h"

struct item {
    int which; /* 0 --segmenter, 1 --adaptor, 2 --polya */
    const char *arg;
    int ok;
};

static const struct item ITEMS[] = {
    {0, "0.75,50,50,150,0.25,5", 1},
    {0, "-1,50,200,250,1,30,560,420", 1},
    {0, "0,50,200,250,1,30,nan,inf", 1},
    {0, "-1,50,200,250,1,30,1e60,-1e60", 1},
    {0, "0.75,50,50,150,0.25,5,1,2", 0},   /* TOP,BOT with STD_SCALE > 0 */
    {0, "-1,50,200,250,1,30", 0},          /* none with STD_SCALE <= 0 */
    {0, "-1,50,200,250,1,30,560", 0},
    {0, "-1,50,200,250,1,30,560,420,1", 0},
    {0, "0.75,50,50,150,0.25", 0},
    {0, "", 0},
    {0, ",", 0},
    {0, "0.75,,50,150,0.25,5", 0},
    {0, "0.75,50,50,150,0.25,5,", 0},
    {0, "0.75, 50,50,150,0.25,5", 0},
    {0, " 0.75,50,50,150,0.25,5", 0},
    {0, "0.75,50,50,150,0.25,5 ", 0},
    {0, "0.75,50x,50,150,0.25,5", 0},
    {0, "0.75,50.0,50,150,0.25,5", 0},
    {0, "0.75,+50,50,150,0.25,5", 0},
    {0, "0.75,0x32,50,150,0.25,5", 0},
    {0, "0.75,50,50,99999999999999999999,0.25,5", 0},
    {0, "0.75,50,50,2147483648,0.25,5", 0},
    {0, "0.75,50,50,-2147483649,0.25,5", 0},
    {0, "nan,50,50,150,0.25,5,1,2", 0},
    {0, "inf,50,50,150,0.25,5", 0},
    {0, "1e60,50,50,150,0.25,5", 0},
    {0, "0.75,50,50,150,nan,5", 0},
    {0, "abc", 0},
    {0, "0.75;50;50;150;0.25;5", 0},
    {0, "-", 0},
    {0, "0.75,-,50,150,0.25,5", 0},
    {1, "0.5,1500,2000,200000,2000", 1},
    {1, "0.7,0,2,1,1", 1},
    {1, "0.5,1500,2000,200000", 0},
    {1, "0.5,1500,2000,200000,2000,1", 0},
    {1, "0.5,1500,2000.0,200000,2000", 0},
    {1, "0.5,1500,2000,200000,2000,", 0},
    {1, "nan,1500,2000,200000,2000", 0},
    {1, "0.5,1500,2e3,200000,2000", 0},
    {1, "", 0},
    {2, "50,200,250,1,30,30,20", 1},
    {2, "50,200,250,0.5,30,-12.5,0", 1},
    {2, "50,200,250,1,30,30", 0},
    {2, "50,200,250,1,30,30,20,1", 0},
    {2, "50,200,250,1,30,30,inf", 0},
    {2, "50,200,250,1,30,nan,20", 0},
    {2, "50.5,200,250,1,30,30,20", 0},
    {2, "50,200,250,1,30,30,20 ", 0},
    {2, ",,,,,,", 0},
};

int main(void) {
    int bad = 0;
    for (size_t i = 0; i < sizeof ITEMS / sizeof ITEMS[0]; i++) {
        double v[SEGOPT_MAX_FIELDS];
        const char *why = NULL;
        const struct item *it = &ITEMS[i];
        const int rc = it->which == 0 ? segopt_segmenter(it->arg, v, &why) : it->which == 1 ? segopt_adaptor(it->arg, v, &why) : segopt_polya(it->arg, v, &why);
        if ((rc == 0) != it->ok || (rc != 0 && (!why || !*why))) {
            fprintf(stderr, "list %d '%s': rc %d, expected %s\n", it->which, it->arg, rc, it->ok ? "taken" : "refused");
            bad++;
        }
    }
    printf("%zu lists, %d wrong\n", sizeof ITEMS / sizeof ITEMS[0], bad);
    return bad ? 1 : 0;
}
