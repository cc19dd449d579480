/* pool.h -- the host program's threads: a persistent pool with a parallel for, and a blocking queue of intrusive nodes.
 * Knows nothing of batches, files or the GPU library (a stand-alone program can link pool.c: tests/host/pool_check.c). */
#ifndef SIGTK_AMD_POOL_H
#define SIGTK_AMD_POOL_H

#include <pthread.h>
#include <stdint.h>

/* parallel for with dynamic scheduling on a persistent pool: fn(ctx, i, tid) for i in [0, n).  A pool belongs to
 * one caller thread (the loader and the writer each own one); its workers sleep between calls. */
typedef void (*pfor_fn)(void *ctx, uint32_t i, int tid);
typedef struct pool pool_t;

pool_t *pool_create(int nthreads);   /* the caller counts as one of them */
void pool_destroy(pool_t *p);
void pfor(pool_t *p, uint32_t n, pfor_fn fn, void *ctx);

/* first in, first out; what is queued embeds a node (as its first member, to be cast back) */
typedef struct qnode {
    struct qnode *next;
} qnode_t;
typedef struct {
    pthread_mutex_t mu;
    pthread_cond_t cv;
    qnode_t *head, *tail;
} queue_t;

void q_init(queue_t *q);
void q_push(queue_t *q, qnode_t *x);
qnode_t *q_pop(queue_t *q);       /* waits for one */
qnode_t *q_try_pop(queue_t *q);   /* NULL when the queue is empty */

#endif
