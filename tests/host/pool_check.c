/* pool_check.c -- sigtk_amd/host/pool.c on its own (tests/test_pool_cpu.py builds the two under -fsanitize=thread):
 * the parallel for visits every index exactly once on pools of 1, 2 and 8 threads, a pool takes 1 000 calls back to back
 * and is destroyed straight after it is created; the queue hands 1 000 nodes from one thread to another in order. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pool.h"

typedef struct {
    uint32_t *hits;   /* per index; each is touched by the one thread that drew it */
    int nthreads, bad_tid;
} visit_t;
static void visit(void *ctx, uint32_t i, int tid) {
    visit_t *v = (visit_t *)ctx;
    v->hits[i]++;
    if (tid < 0 || tid >= v->nthreads) __atomic_store_n(&v->bad_tid, 1, __ATOMIC_RELAXED);
}

static int check_pool(int nthreads) {
    const uint32_t sizes[5] = {0, 1, (uint32_t)nthreads - 1, (uint32_t)nthreads + 1, 10000};
    int wrong = 0;
    visit_t v = {(uint32_t *)calloc(10000, sizeof(uint32_t)), nthreads, 0};
    if (!v.hits) return 1;
    pool_destroy(pool_create(nthreads));   /* destroyed before any worker has had a call */
    pool_t *p = pool_create(nthreads);
    for (int s = 0; s < 5; s++) {
        memset(v.hits, 0, 10000 * sizeof(uint32_t));
        pfor(p, sizes[s], visit, &v);
        for (uint32_t i = 0; i < 10000; i++) wrong += v.hits[i] != (i < sizes[s] ? 1u : 0u);
    }
    memset(v.hits, 0, 10000 * sizeof(uint32_t));
    for (int k = 0; k < 1000; k++) pfor(p, (uint32_t)nthreads + 1, visit, &v);
    for (uint32_t i = 0; i < 10000; i++) wrong += v.hits[i] != (i < (uint32_t)nthreads + 1 ? 1000u : 0u);
    pool_destroy(p);
    wrong += v.bad_tid;
    free(v.hits);
    return wrong;
}

typedef struct {
    qnode_t link;   /* first: cast back from the node */
    int serial;
} item_t;
static void *consumer(void *q_) {
    long wrong = 0;
    for (int k = 0; k < 1000; k++) {
        item_t *it = (item_t *)q_pop((queue_t *)q_);
        wrong += it->serial != k;
    }
    return (void *)wrong;
}
static int check_queue(void) {
    static item_t items[1000];
    queue_t q;
    pthread_t th;
    void *res = NULL;
    q_init(&q);
    int wrong = q_try_pop(&q) != NULL;
    if (pthread_create(&th, NULL, consumer, &q) != 0) return 1;
    for (int k = 0; k < 1000; k++) {
        items[k].serial = k;
        q_push(&q, &items[k].link);
    }
    pthread_join(th, &res);
    wrong += (int)(long)res + (q_try_pop(&q) != NULL);
    q_push(&q, &items[0].link);
    wrong += q_try_pop(&q) != &items[0].link;
    return wrong;
}

int main(void) {
    const int wrong = check_pool(1) + check_pool(2) + check_pool(8) + check_queue();
    printf("pools of 1, 2 and 8 threads and the queue: %d wrong\n", wrong);
    return wrong ? 1 : 0;
}
